"""GPU: nvrx_histogram_history_scores_compact against the compact host twin
(``histograms.compact_history_scores``) over every case of ``_histogram_compact_cases`` in SCORE,
SCORE with tail_calls, UPDATE, SCORE|UPDATE and SCORE|UPDATE with tail_calls: integers equal, f64
bit patterns equal (NaN as NaN), the whole history tensor equal, sentinel slots and a guard region
behind it included; no tolerance.  Then the relations: to the dense entry on the dense expansion
while nothing folds, to ``ops.segment_history_scores_compact_ragged`` on samples with the same
counts (a folding case included), fused against score-then-update, run to run, and a captured
graph against the eager call."""
import numpy as np
import pytest
import torch

import _histogram_compact_cases as C
from nvidia_resiliency_ext.straggler import histograms, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -7
GUARD = 0x5E
SCORE, UPDATE = 1, 2
BOTH = SCORE | UPDATE
RUNS = ((SCORE, False), (SCORE, True), (UPDATE, False), (BOTH, False), (BOTH, True))
SUMS = ("tail_ns", "total_ns", "base_tail_ns", "base_total_ns")
CASES = C.cases()


def dev(a, dt=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(DEV)


def opt(v, dt):
    return None if v is None else torch.as_tensor(np.asarray(v), dtype=dt).to(DEV)


def guarded_chist(ch):
    """A device copy of a compact history with 64 guard bytes behind it: (the view, the whole)."""
    whole = torch.full((ch.size + C.CB,), GUARD, dtype=torch.uint8, device=DEV)
    view = whole[:ch.size].view(ch.shape)
    view.copy_(torch.from_numpy(ch).to(DEV))
    return view, whole


def sentinel_out(R):
    i = lambda: torch.full((R,), SENT, dtype=torch.int64, device=DEV)  # noqa: E731
    return ops.HistoryTailScores(torch.full((R,), float(SENT), dtype=torch.float64, device=DEV),
                                 i(), i(), i(), i(), torch.full((R,), 9, dtype=torch.uint8, device=DEV))


def untouched(out):
    R = out.score.numel()
    return (out.score.cpu().tolist() == [float(SENT)] * R and out.strag.cpu().tolist() == [9] * R and
            all(getattr(out, n).cpu().tolist() == [SENT] * R for n in SUMS))


def kwargs(c):
    return dict(hist_index=opt(c.hist_index, torch.int32), hist_stride=c.stride,
                col_valid=opt(c.col_valid, torch.uint8), skip_rows=opt(c.skip_rows, torch.uint8),
                permille=c.pm, score_thr=C.THR)


def run(c, d_counts, d_chist, mode, calls, kw):
    out = sentinel_out(c.R)
    folded = torch.full((c.R,), SENT, dtype=torch.int64, device=DEV)
    tc = torch.full((c.R * c.K + 4,), SENT, dtype=torch.int32, device=DEV) if calls else None
    res, f = ops.histogram_history_scores_compact(
        d_counts, d_chist, score=bool(mode & SCORE), update=bool(mode & UPDATE),
        tail_calls=tc[:c.R * c.K].view(c.R, c.K) if calls else False, out=out, folded=folded, **kw)
    assert tc is None or tc[-4:].cpu().tolist() == [SENT] * 4
    assert (f is folded) if mode & UPDATE else (f is None)
    return res, out, folded


def assert_twin(res, twin, calls):
    for n in SUMS:
        assert np.array_equal(getattr(res, n).cpu().numpy().view(np.uint64), getattr(twin, n)), n
    assert res.score.cpu().numpy().tobytes() == twin.score.tobytes()
    assert res.strag.cpu().numpy().astype(bool).tolist() == twin.stragglers.tolist()
    if calls:
        assert np.array_equal(res.tail_calls.cpu().numpy().view(np.uint32), twin.tail_calls)
    else:
        assert res.tail_calls is None


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_equals_the_twin_in_every_mode(c):
    twin = C.expected(c.name)
    d_counts, kw = dev(c.counts), kwargs(c)
    for mode, calls in RUNS:
        d_chist, whole = guarded_chist(c.chist0)
        res, out, folded = run(c, d_counts, d_chist, mode, calls, kw)
        assert whole[-C.CB:].cpu().tolist() == [GUARD] * C.CB
        # the whole tensor, sentinel slots included
        assert np.array_equal(d_chist.cpu().numpy(), twin.hist if mode & UPDATE else c.chist0), (mode, calls)
        if mode & UPDATE:
            assert np.array_equal(folded.cpu().numpy().view(np.uint64), twin.folded)
        else:
            assert folded.cpu().tolist() == [SENT] * c.R
        if mode & SCORE:
            assert_twin(res, twin, calls)
        else:
            assert untouched(out) and res.tail_calls is None
    assert np.array_equal(d_counts.cpu().numpy().view(np.uint32), c.counts)


def test_the_cases_hit_what_they_aim_at():
    """The twin's own view of the directed elements: what folds, what saturates, what is left."""
    by = {s.name: C.expected("elem_" + s.name) for s in C.SPECS}
    el = lambda n: histograms.compact_to_dense(by[n].hist[:, :1])[0, 0]  # noqa: E731
    assert np.array_equal(by["no_samples"].hist[0, 0], C.case("elem_no_samples").chist0[0, 0])
    assert by["empty_history"].threshold_bucket[0, 0] == -1 and el("empty_history")[5] == 3
    assert el("full_new_below")[10] == 5 + 5 and el("full_new_above")[120] == 5 + 4
    assert el("n11_one_more_than_fits")[2] == 1 and el("n11_one_more_than_fits")[103] == 11 + 4
    assert el("two_free_three_new")[30] == 9 + 1 + 3 and el("two_free_three_new")[40] == 0
    assert el("fold_sum_needs_64_bits")[120] == C.U32 and el("kept_entry_saturates")[50] == C.U32
    assert [by[n].threshold_bucket[0, 0] for n in ("buckets_0_3_4", "buckets_63_64", "bucket_239",
                                                    "wide_buckets", "T_inside_a_lane",
                                                    "T_is_the_highest_bucket")] == [4, 63, 0, 238, 9, 60]
    # the spec sits at four columns; the other columns fold nothing in this case
    assert int(by["fold_sum_needs_64_bits"].folded[0]) >= 4 * 3 * 0xFFFFFFF0 > 2 ** 32
    assert len({c.pm for c in CASES}) >= 6 and {0, 500, 990, 1000} <= {c.pm for c in CASES}


def test_saturating_fold_takes_its_sum_in_64_bits():
    c = C.build("one", 1, 1, lambda r, k: [s.name for s in C.SPECS].index("fold_sum_needs_64_bits"), 950)
    d_chist = dev(c.chist0, np.uint8)
    _, _, folded = run(c, dev(c.counts), d_chist, UPDATE, False, kwargs(c))
    got = histograms.compact_to_dense(d_chist.cpu().numpy())[0, 0]
    assert got[120] == 0xFFFFFFFF and got.sum() == 11 * 5 + 0xFFFFFFFF
    assert folded.cpu().numpy().view(np.uint64).tolist() == [3 * 0xFFFFFFF0]
    # the same through from_dense: twelve buckets of 1, then 0x10 + three bins above them
    h = np.zeros((1, 1, C.BINS), np.uint32)
    h[0, 0, 10:21] = 1
    h[0, 0, [120, 130, 140, 150]] = (0x10, 0xFFFFFFF0, 0xFFFFFFF0, 0xFFFFFFF0)
    ch, f = ops.compact_history_from_dense(dev(h))
    want, wf = histograms.compact_from_dense(h)
    assert np.array_equal(ch.cpu().numpy(), want)
    assert f.cpu().numpy().view(np.uint64).tolist() == wf.tolist() == [3 * 0xFFFFFFF0]
    assert histograms.compact_to_dense(want)[0, 0, 120] == 0xFFFFFFFF


def test_three_chained_intervals_equal_the_dense_entry_bit_for_bit():
    R, K = 3, 37
    rng = np.random.default_rng(11)
    d_chist = torch.zeros((R, K, C.CB), dtype=torch.uint8, device=DEV)
    d_hist = torch.zeros((R, K, C.BINS), dtype=torch.int32, device=DEV)
    valid = np.ones(K, np.uint8)
    valid[[3, 16]] = 0
    kw = dict(permille=900, score_thr=C.THR, col_valid=opt(valid, torch.uint8), tail_calls=True)
    for i in range(3):
        counts = C.clustered(rng, R, K)
        counts[i % R, (5 * i) % K] = 0  # an element without samples
        d_counts = dev(counts)
        got, folded = ops.histogram_history_scores_compact(d_counts, d_chist, **kw)
        want = ops.histogram_history_scores(d_counts, d_hist, **kw)
        assert folded.cpu().tolist() == [0] * R
        for n in SUMS + ("score", "strag", "tail_calls"):
            assert same_bits(getattr(got, n), getattr(want, n)), (i, n)
        assert same_bits(ops.compact_history_to_dense(d_chist), d_hist)
        assert i == 0 or not np.isnan(got.score.cpu().numpy()).any()
    assert histograms.compact_is_canonical(d_chist.cpu().numpy()).all()


def ragged(counts, rng):
    """Samples whose ``histograms.segment_counts`` are ``counts`` ([R, K, 240], small): keys,
    seg_off, seg_len."""
    edges = histograms.edges_keys()[:C.BINS]  # a key of every bucket: its lower edge
    R, K, _ = counts.shape
    keys, off, lens = [], [], []
    n = 0
    for g in range(R * K):
        c = counts.reshape(R * K, C.BINS)[g]
        run = rng.permutation(np.repeat(edges, c).astype(np.uint32))
        off.append(n)
        lens.append(run.size)
        keys.append(run)
        n += run.size
    keys = np.concatenate(keys + [np.zeros(1, np.uint32)])
    return keys, np.asarray(off, np.int64), np.asarray(lens, np.int32)


@pytest.mark.parametrize("fold", [False, True])
def test_record_stream_entry_leaves_the_same_history_and_outputs(fold):
    R, K = 2, 21
    rng = np.random.default_rng(23 + fold)
    counts = C.clustered(rng, R, K, peak=60)
    chist0 = histograms.compact_from_dense(C.clustered(rng, R, K, peak=500))[0]
    counts[1, 4] = 0
    if fold:  # full elements hit in new buckets below, between and above, and two free of three
        for k, s in ((0, "full_new_below"), (7, "full_new_between"), (16, "full_new_above"),
                     (20, "two_free_three_new"), (9, "n11_one_more_than_fits")):
            spec = next(x for x in C.SPECS if x.name == s)
            counts[0, k], chist0[0, k] = C.dense(spec.cur), C.element(spec.hist)
    keys, off, lens = ragged(counts, rng)
    assert np.array_equal(histograms.segment_counts(keys, off, lens, K), counts)
    twin = histograms.compact_history_scores(counts, chist0, 950, score_thr=C.THR)
    assert bool(twin.folded.any()) == fold
    kw = dict(permille=950, score_thr=C.THR, tail_calls=True)
    a_h, b_h = dev(chist0, np.uint8), dev(chist0, np.uint8)
    a, a_f = ops.histogram_history_scores_compact(dev(counts), a_h, **kw)
    b, b_f = ops.segment_history_scores_compact_ragged(dev(keys), dev(off, np.int64), dev(lens), K,
                                                       int(lens.max()), b_h, **kw)
    for n in SUMS + ("score", "strag", "tail_calls"):
        assert same_bits(getattr(a, n), getattr(b, n)), n
    assert torch.equal(a_h, b_h) and torch.equal(a_f, b_f)
    assert_twin(a, twin, True)
    assert np.array_equal(a_h.cpu().numpy(), twin.hist)
    assert np.array_equal(a_f.cpu().numpy().view(np.uint64), twin.folded)


@pytest.mark.parametrize("name", ["R3_K37", "all_three", "elem_fold_sum_needs_64_bits"])
def test_fused_equals_score_then_update_and_two_runs_agree(name):
    c = C.case(name)
    d_counts, kw = dev(c.counts), kwargs(c)
    ha, hb, hc = (dev(c.chist0, np.uint8) for _ in range(3))
    a, _, fa = run(c, d_counts, ha, BOTH, True, kw)
    b, _, fb = run(c, d_counts, hb, BOTH, True, kw)
    s, _, _ = run(c, d_counts, hc, SCORE, True, kw)
    assert torch.equal(hc, dev(c.chist0, np.uint8))
    _, _, fc = run(c, d_counts, hc, UPDATE, False, kw)
    for n in SUMS + ("score", "strag", "tail_calls"):
        assert same_bits(getattr(a, n), getattr(b, n)), n
        assert same_bits(getattr(a, n), getattr(s, n)), n
    assert torch.equal(ha, hb) and torch.equal(fa, fb)
    assert torch.equal(ha, hc) and torch.equal(fa, fc)


def test_graph_capture_and_replay_equals_the_eager_call():
    c = C.case("all_three")
    twin = C.expected(c.name)
    d_counts, kw = dev(c.counts), kwargs(c)
    d_chist = dev(c.chist0, np.uint8)
    out = sentinel_out(c.R)
    folded = torch.full((c.R,), SENT, dtype=torch.int64, device=DEV)
    calls = torch.full((c.R, c.K), SENT, dtype=torch.int32, device=DEV)

    def launch():
        return ops.histogram_history_scores_compact(d_counts, d_chist, tail_calls=calls, out=out,
                                                    folded=folded, **kw)[0]

    launch()  # the kernels are loaded before the capture
    torch.cuda.synchronize()
    eager = d_chist.clone()
    d_chist.copy_(dev(c.chist0, np.uint8))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = launch()
    d_chist.copy_(dev(c.chist0, np.uint8))  # the history is restored before the replay
    for t in (out.tail_ns, out.total_ns, out.base_tail_ns, out.base_total_ns, calls, folded):
        t.fill_(SENT)
    g.replay()
    torch.cuda.synchronize()
    assert_twin(res, twin, True)
    assert np.array_equal(folded.cpu().numpy().view(np.uint64), twin.folded)
    assert torch.equal(d_chist, eager) and np.array_equal(eager.cpu().numpy(), twin.hist)


def test_wrapper_rejects_a_history_of_the_wrong_shape_or_type():
    c = C.case("R1_K1")
    for bad in (torch.zeros((c.R, c.K, 60), dtype=torch.uint8, device=DEV),
                torch.zeros((c.R, c.K, 16), dtype=torch.int32, device=DEV)):
        with pytest.raises(ValueError, match="chist"):
            ops.histogram_history_scores_compact(dev(c.counts), bad, permille=c.pm)
