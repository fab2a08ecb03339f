"""GPU: aging through the reporter and the Detector, on a small reporter (R 3, K 5, cap 16) over
five intervals of hand-made record streams whose durations drift from interval to interval, so
that halving evicts entries: ``MatrixReporter.age_tail_history`` for each ``history`` against the
host twins; ``half_life=2`` over five ``individual_tail_scores_records`` calls, dense and compact,
against the host chain with aging before calls 3 and 5; what counts towards the half life and what
restarts the count; ``Detector.age_tail_history`` on a hand-filled history."""
import numpy as np
import pytest
import torch

from nvidia_resiliency_ext.straggler import batch, histograms, straggler

pytestmark = pytest.mark.gpu

R, K, CAP, PM, THR = 3, 5, 16, 900, 0.9
NIV = 5


@pytest.fixture(scope="module")
def intervals():
    """Per interval (recs [n, 2] int32 {slot, ns}, rec_off [R + 1] int64) on the device: each rank
    20..39 records per kernel (more than cap), durations around a per-kernel base that moves one
    to two buckets per interval, with a few slow calls."""
    rng = np.random.default_rng(2024)
    out = []
    for i in range(NIV):
        streams = []
        for r in range(R):
            slot = np.repeat(np.arange(K), rng.integers(20, 40, K))
            rng.shuffle(slot)
            base = 1000.0 * (1 + slot) * 1.2 ** i
            ns = base * rng.choice([1.0, 1.05, 1.3, 4.0], slot.size, p=[0.6, 0.2, 0.15, 0.05])
            streams.append(np.stack([slot, ns.astype(np.int64)], 1).astype(np.int32))
        off = np.concatenate([[0], np.cumsum([s.shape[0] for s in streams])]).astype(np.int64)
        out.append((torch.from_numpy(np.concatenate(streams)).cuda(), torch.from_numpy(off).cuda()))
    return out


def buckets(rep):
    """The buckets the reporter's last record-stream call laid out, on the host."""
    seg_off, seg_len, out_ns, _ = rep._rtail["bucket"]
    return (out_ns.cpu().numpy().view(np.uint32), seg_off.cpu().numpy(), seg_len.cpu().numpy(), K)


def twin(kind, args, h, absorb):
    """One call on the host: the scores and the history afterwards."""
    f = (histograms.segment_compact_history_scores if kind == "compact"
         else histograms.segment_history_scores)
    args = args + (h, PM, CAP)
    if absorb != "healthy":
        res = f(*args, update=absorb == "always", score_thr=THR)
        return res, res.hist if absorb == "always" else h
    s = f(*args, update=False, score_thr=THR)
    u = f(*args, score=False, skip_rows=s.stragglers)
    if kind == "compact":
        s.folded = u.folded
    return s, u.hist


def empty(kind):
    return (np.zeros((R, K, histograms.CHIST_BYTES), np.uint8) if kind == "compact"
            else np.zeros((R, K, histograms.BINS), np.uint32))


def age(kind, h, shift=1):
    return histograms.compact_age(h, shift)[0] if kind == "compact" else histograms.history_age(h, shift)


def device_history(rep, kind):
    if kind == "compact":
        return rep.compact_tail_history().cpu().numpy()
    return rep._htail["hist"].cpu().numpy().view(np.uint32)


def run(rep, kind, iv, absorb="healthy", **kw):
    return rep.individual_tail_scores_records(*iv, permille=PM, threshold=THR, absorb=absorb,
                                              history=kind, **kw)


def fill(rep, ivs, kinds=("dense", "compact")):
    """Absorb the intervals into the reporter's histories; the host's copies."""
    h = {k: empty(k) for k in kinds}
    for iv in ivs:
        for k in kinds:
            run(rep, k, iv, "always")
            h[k] = twin(k, buckets(rep), h[k], "always")[1]
    return h


def test_before_first_use_nothing_is_allocated(intervals):
    rep = batch.MatrixReporter(R, K, cap=CAP)
    for kind in batch.HISTORY_KINDS:
        res = rep.age_tail_history(history=kind)
        assert res.evicted is None and res.full is None
    assert rep._htail is None and rep._ctail is None and rep.compact_tail_history() is None
    # a reporter with the dense history only: "both" ages it and skips the compact one
    h = fill(rep, intervals[:1], kinds=("dense",))
    res = rep.age_tail_history(history="both")
    assert res.evicted is None and res.full is None and rep._ctail is None
    assert np.array_equal(device_history(rep, "dense"), age("dense", h["dense"]))
    res = rep.age_tail_history(history="compact")
    assert res.evicted is None and rep._ctail is None


@pytest.mark.parametrize("shift", [1, 3])
@pytest.mark.parametrize("kind", batch.HISTORY_KINDS)
def test_age_tail_history_equals_the_twins(intervals, kind, shift):
    rep = batch.MatrixReporter(R, K, cap=CAP)
    h = fill(rep, intervals[:3])
    assert np.array_equal(histograms.compact_to_dense(h["compact"]), h["dense"])  # nothing folded
    res = rep.age_tail_history(shift, history=kind)
    want_c, ev, fu = histograms.compact_age(h["compact"], shift)
    if kind in ("compact", "both"):
        assert res.evicted.dtype == res.full.dtype == np.uint64
        assert np.array_equal(res.evicted, ev) and np.array_equal(res.full, fu)
        assert ev.sum() > 0  # the drift left entries a halving evicts
        assert np.array_equal(device_history(rep, "compact"), want_c)
    else:
        assert res.evicted is None and res.full is None
        assert np.array_equal(device_history(rep, "compact"), h["compact"])
    want_d = histograms.history_age(h["dense"], shift) if kind in ("dense", "both") else h["dense"]
    assert np.array_equal(device_history(rep, "dense"), want_d)
    if kind == "both":  # the two histories stay bit-identical through aging
        assert np.array_equal(histograms.compact_to_dense(device_history(rep, "compact")),
                              device_history(rep, "dense"))


@pytest.mark.parametrize("absorb", ["healthy", "always"])
@pytest.mark.parametrize("kind", ["dense", "compact"])
def test_half_life_two_over_five_calls_equals_the_host_chain(intervals, kind, absorb):
    rep = batch.MatrixReporter(R, K, cap=CAP)
    h = empty(kind)
    scored = 0
    for i, iv in enumerate(intervals):
        got = run(rep, kind, iv, absorb, half_life=2)
        if i in (2, 4):  # two absorbing calls counted: age first
            h = age(kind, h)
        want, h = twin(kind, buckets(rep), h, absorb)
        assert got.score.tobytes() == want.score.tobytes(), i
        assert got.stragglers.tolist() == want.stragglers.tolist()
        for n in ("tail_ns", "total_ns", "base_tail_ns", "base_total_ns"):
            assert np.array_equal(getattr(got, n), getattr(want, n)), (i, n)
        if kind == "compact":
            assert np.array_equal(got.folded, want.folded)
        assert np.array_equal(device_history(rep, kind), h), i
        scored += int(np.isfinite(got.score).sum())
    assert scored > 0
    # and the chain without aging ends somewhere else: the test can tell the difference
    plain = batch.MatrixReporter(R, K, cap=CAP)
    for iv in intervals:
        run(plain, kind, iv, absorb)
    assert not np.array_equal(device_history(plain, kind), h)


@pytest.mark.parametrize("kind", ["dense", "compact"])
def test_what_counts_towards_the_half_life_and_what_restarts_it(intervals, kind):
    other = "compact" if kind == "dense" else "dense"
    # absorb="never" does not count, and neither does a call on the other history
    rep = batch.MatrixReporter(R, K, cap=CAP)
    h = empty(kind)
    plan = [("always", False), ("never", False), ("always", False), ("never", True), ("always", False)]
    for iv, (absorb, aged) in zip(intervals, plan):
        run(rep, other, iv, "always", half_life=2)
        run(rep, kind, iv, absorb, half_life=2)
        if aged:  # the fourth call finds two absorbing calls
            h = age(kind, h)
        h = twin(kind, buckets(rep), h, absorb)[1]
        assert np.array_equal(device_history(rep, kind), h), (absorb, aged)
    # half_life=None never ages, however many calls were counted
    run(rep, kind, intervals[0], "always")
    h = twin(kind, buckets(rep), h, "always")[1]
    assert np.array_equal(device_history(rep, kind), h)
    # reset_tail_history restarts the count: without it the first call after it would age
    rep = batch.MatrixReporter(R, K, cap=CAP)
    for iv in intervals[:2]:
        run(rep, kind, iv, "always", half_life=2)
    rep.reset_tail_history()
    h = empty(kind)
    for iv in intervals[2:4]:
        run(rep, kind, iv, "always", half_life=2)
        h = twin(kind, buckets(rep), h, "always")[1]
    assert np.array_equal(device_history(rep, kind), h)
    # age_tail_history restarts the count of the history it aged
    rep.age_tail_history(history=kind)
    h = age(kind, h)
    run(rep, kind, intervals[4], "always", half_life=2)
    h = twin(kind, buckets(rep), h, "always")[1]
    assert np.array_equal(device_history(rep, kind), h)


def test_individual_tail_scores_shares_the_dense_count(intervals):
    rep = batch.MatrixReporter(R, K, cap=CAP)
    h = fill(rep, intervals[:2], kinds=("dense",))["dense"]  # two absorbing record-stream calls
    counts = torch.zeros((R, K, histograms.BINS), dtype=torch.int32, device="cuda")
    counts[:, :, 100] = 3
    rep.individual_tail_scores(counts, permille=PM, threshold=THR, absorb="always", half_life=2)
    want = histograms.history_scores(counts.cpu().numpy(), histograms.history_age(h, 1), PM,
                                     score_thr=THR).hist
    assert np.array_equal(device_history(rep, "dense"), want)


def test_arguments_are_checked(intervals):
    rep = batch.MatrixReporter(R, K, cap=CAP)
    for bad in (0, 32, 1.5, True):
        with pytest.raises(ValueError, match="shift"):
            rep.age_tail_history(bad)
    with pytest.raises(ValueError, match="history"):
        rep.age_tail_history(history="sparse")
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="half_life"):
            run(rep, "dense", intervals[0], half_life=bad)
        with pytest.raises(ValueError, match="half_life"):
            rep.individual_tail_scores(None, half_life=bad)
    assert rep._htail is None and rep._ctail is None  # refused before anything is allocated
    rep.exchange = True  # as a reporter over kernel shards
    with pytest.raises(NotImplementedError, match="exchange=True"):
        rep.age_tail_history()


def test_detector_age_tail_history():
    saved = getattr(straggler.Detector, "_tail_history", None)
    try:
        th = straggler._TailHistory()
        straggler.Detector._tail_history = th
        straggler.Detector.age_tail_history()  # nothing before the first interval
        assert th.hist is None
        rng = np.random.default_rng(5)
        host = rng.integers(0, 1 << 32, (1, 64, histograms.BINS), dtype=np.uint64).astype(np.uint32)
        host[0, 0, 0], host[0, 63, 239], host[0, 1] = 2 ** 32 - 1, 2 ** 32 - 1, 0
        th.hist = torch.from_numpy(host.view(np.int32)).cuda()
        th.intervals = 4
        straggler.Detector.age_tail_history()
        assert np.array_equal(th.hist.cpu().numpy().view(np.uint32), histograms.history_age(host, 1))
        straggler.Detector.age_tail_history(shift=5)
        assert np.array_equal(th.hist.cpu().numpy().view(np.uint32), histograms.history_age(host, 6))
        assert th.intervals == 4  # left alone
        with pytest.raises(ValueError, match="shift"):
            straggler.Detector.age_tail_history(0)
    finally:
        if saved is None:
            del straggler.Detector._tail_history
        else:
            straggler.Detector._tail_history = saved
