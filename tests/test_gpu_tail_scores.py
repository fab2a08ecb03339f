"""GPU: the tail-score kernels (nvrx_histogram_sum / _tail_threshold / _tail_scores) against the
definition in plain Python integers (``_tail_ref``): integers equal, f64 bit patterns equal (NaN
as NaN), no tolerance.  Every output is pre-filled with a sentinel and must be written in full."""
import numpy as np
import pytest
import torch

import _tail_ref as REF
import oracle as O
from nvidia_resiliency_ext.straggler import batch, ops

pytestmark = pytest.mark.gpu

BINS = 240
DEV = "cuda"
SENT = -7
U64 = np.uint64


def make_counts(R, K, seed):
    """u32 counts [R, K, 240]: clustered kernels (2-3 buckets), spread ones, clustered ones with
    a tail on every 5th row, and the hand-made columns / rows the shape has room for."""
    rng = np.random.default_rng(seed)
    c = np.zeros((R, K, BINS), np.uint32)
    for k in range(K):
        base = int(rng.integers(40, 200))
        if k % 3 == 1:  # spread
            dense = rng.random((R, BINS)) < 0.3
            c[:, k] = rng.integers(0, 2000, size=(R, BINS)) * dense
        else:           # clustered
            for j in range(int(rng.integers(2, 4))):
                c[:, k, base + j] = rng.integers(1, 400, size=R)
            if k % 3 == 2:
                c[::5, k, base + 6] = rng.integers(1, 40, size=len(range(0, R, 5)))
    if K >= 2:  # counts the int32 view shows negative
        c[0, 1, 77], c[R - 1, 1, 78], c[R // 2, 1, 90] = 0x80000000, 0xFFFFFFFF, 0x80000001
    if K >= 5:
        c[:, 3] = 0                       # a kernel nobody ran
        c[:, 4] = 0
        c[:, 4, 239] = rng.integers(1, 9, size=R)  # a fleet in bucket 239 alone: T = 239
    if R >= 3:
        c[1] = 0                          # a rank without samples: NaN, never flagged
    return c


def dev_counts(c):
    return torch.from_numpy(c.view(np.int32)).to(DEV)


def u64_list(t):
    return t.cpu().numpy().view(U64).tolist()


def run_sum(d, accumulate=False, out=None):
    R, K = d.shape[:2]
    if out is None:
        out = torch.full((K, BINS), SENT, dtype=torch.int64, device=DEV)
    return ops.histogram_sum(d, out=out, accumulate=accumulate)


def run_threshold(fleet, pm, col_valid=None):
    K = fleet.shape[0]
    thr = torch.full((K,), SENT, dtype=torch.int32, device=DEV)
    sums = torch.full((2,), SENT, dtype=torch.int64, device=DEV)
    cv = None if col_valid is None else torch.tensor(col_valid, dtype=torch.uint8, device=DEV)
    return ops.histogram_tail_threshold(fleet, pm, col_valid=cv, thr=thr, fleet_sums=sums)


def run_scores(d, thr, sums, score_thr, thr_index=None, calls=False):
    R, K = d.shape[:2]
    out = ops.TailScores(torch.full((R,), float(SENT), dtype=torch.float64, device=DEV),
                         torch.full((R,), SENT, dtype=torch.int64, device=DEV),
                         torch.full((R,), SENT, dtype=torch.int64, device=DEV),
                         torch.full((R,), 9, dtype=torch.uint8, device=DEV))
    tc = torch.full((R, K), SENT, dtype=torch.int32, device=DEV) if calls else False
    ti = None if thr_index is None else torch.tensor(thr_index, dtype=torch.int32, device=DEV)
    return ops.histogram_tail_scores(d, thr, sums, score_thr=score_thr, thr_index=ti,
                                     tail_calls=tc, out=out)


def assert_rows(res, rows, calls):
    assert u64_list(res.tail_ns) == [r["tail_ns"] for r in rows]
    assert u64_list(res.total_ns) == [r["total_ns"] for r in rows]
    assert [REF.bits(s) for s in res.score.cpu().tolist()] == [REF.bits(r["score"]) for r in rows]
    assert res.strag.cpu().tolist() == [int(r["strag"]) for r in rows]
    if calls:
        got = res.tail_calls.cpu().numpy().view(np.uint32).tolist()
        assert got == [r["calls"] for r in rows]
    else:
        assert res.tail_calls is None


def check_all(c, pm, score_thr=0.9, col_valid=None):
    """The three calls over counts c against the reference; returns the reference rows."""
    F, T, sums, rows = REF.full(c.tolist(), pm, score_thr, col_valid)
    d = dev_counts(c)
    fleet = run_sum(d)
    assert u64_list(fleet.view(-1)) == [v for f in F for v in f]  # all 240 bins of every kernel
    thr, s = run_threshold(fleet, pm, col_valid)
    assert thr.cpu().tolist() == T  # the -1s included
    assert tuple(u64_list(s)) == sums
    assert_rows(run_scores(d, thr, s, score_thr), rows, False)
    assert_rows(run_scores(d, thr, s, score_thr, calls=True), rows, True)
    return T, sums, rows


SHAPES = [(R, K) for R in (1, 2, 3, 64, 257) for K in (1, 2, 5, 67)] + [(1030, 3), (2, 2049)]
PMS = (990, 950, 500, 999)


@pytest.mark.parametrize("R,K", SHAPES)
def test_three_calls_equal_the_reference(R, K):
    i = SHAPES.index((R, K))
    T, sums, rows = check_all(make_counts(R, K, seed=1000 + i), PMS[i % len(PMS)])
    if K >= 5:
        assert T[3] == -1 and T[4] == 239
    if R >= 3:
        assert rows[1]["score"] != rows[1]["score"] and not rows[1]["strag"]


@pytest.mark.parametrize("R,K", [(3, 5), (64, 67)])
def test_permille_ends(R, K):
    c = make_counts(R, K, seed=7)
    _, _, rows = check_all(c, 1000)  # T = the fleet's top bucket: no tail, every score exactly 1.0
    assert all(r["tail_ns"] == 0 for r in rows)
    assert [r["score"] for i, r in enumerate(rows) if i != 1] == [1.0] * (R - 1)
    check_all(c, 0)


@pytest.mark.parametrize("R,K", [(3, 5), (64, 67)])
def test_col_valid_with_zeros(R, K):
    c = make_counts(R, K, seed=8)
    valid = [int(k % 3 != 0) for k in range(K)]
    T, _, _ = check_all(c, 990, col_valid=valid)
    assert all(T[k] == -1 for k in range(0, K, 3))


def test_weightless_fleet_gives_nan():
    c = np.zeros((3, 2, BINS), np.uint32)
    c[:, :, 0] = 5  # bucket 0 weighs 0: fleet_total == 0
    _, sums, rows = check_all(c, 500)
    assert sums == (0, 0) and all(r["score"] != r["score"] and not r["strag"] for r in rows)


def test_sums_above_2_53():
    c = np.zeros((2, 3, BINS), np.uint32)
    c[0, 0, 230], c[1, 0, 231], c[0, 1, 9], c[1, 1, 11], c[:, 2, 236] = 0xFFFFFFFF, 0xFFFFFFFD, 1, 3, 0xFFFFFFF1
    _, sums, _ = check_all(c, 500)
    assert sums[1] > 2 ** 53 and float(sums[1]) != sums[1]


@pytest.mark.parametrize("R,K", [(3, 5), (257, 67)])
def test_thr_index_permutation_with_skips(R, K):
    # the rows hold K kernels out of a fleet of U = K + 2, in another order; some are not taken
    U = K + 2
    fleet_counts = make_counts(4, U, seed=21)
    F, T, sums, _ = REF.full(fleet_counts.tolist(), 950, 0.9)
    rng = np.random.default_rng(22)
    index = rng.permutation(U)[:K].astype(np.int64)
    index[::4] = -1
    c = make_counts(R, K, seed=23)
    rows = REF.scores(c.tolist(), T, sums, 0.9, thr_index=index.tolist())
    thr, s = run_threshold(run_sum(dev_counts(fleet_counts)), 950)
    assert thr.cpu().tolist() == T
    d = dev_counts(c)
    assert_rows(run_scores(d, thr, s, 0.9, thr_index=index.tolist()), rows, False)
    assert_rows(run_scores(d, thr, s, 0.9, thr_index=index.tolist(), calls=True), rows, True)
    assert all(r["calls"][k] == 0 for r in rows for k in range(0, K, 4))


@pytest.mark.parametrize("R,K", [(3, 5), (257, 67), (1030, 3)])
def test_accumulate_adds(R, K):
    a, b = make_counts(R, K, seed=31), make_counts(R, K, seed=32)
    Fa, Fb = REF.fleet_of(a.tolist()), REF.fleet_of(b.tolist())
    fleet = run_sum(dev_counts(a))
    run_sum(dev_counts(b), accumulate=True, out=fleet)
    assert u64_list(fleet.view(-1)) == [x + y for fa, fb in zip(Fa, Fb) for x, y in zip(fa, fb)]
    with pytest.raises(ValueError, match="accumulate"):
        ops.histogram_sum(dev_counts(a), accumulate=True)


# ---------------------------------------------------------------- MatrixReporter, end to end
E2E = dict(R=8, K=5, S=512, slow=3, every=10, factor=3, pm=950, thr=0.9)


def e2e_keys():
    """synth keys without a synthetic straggler; one rank 3x slower on every 10th sample."""
    R, K, S = E2E["R"], E2E["K"], E2E["S"]
    ns = O.gen_matrix(R, K, S, straggler=np.zeros(R, np.uint8)).reshape(R, K, S).astype(np.uint64)
    ns[E2E["slow"], :, ::E2E["every"]] *= E2E["factor"]
    return ns.astype(np.uint32)


def test_matrix_reporter_end_to_end():
    R, K, S, slow = E2E["R"], E2E["K"], E2E["S"], E2E["slow"]
    keys = e2e_keys()
    counts = [[REF.hist_of(keys[r, k]) for k in range(K)] for r in range(R)]
    _, T, sums, rows = REF.full(counts, E2E["pm"], E2E["thr"])
    ns = torch.from_numpy(keys.view(np.int32)).to(DEV)
    rep = batch.MatrixReporter(R, K, cap=8192, thr_rel=E2E["thr"], device=DEV)
    h = rep.histograms(ns, S)
    assert h.cpu().numpy().view(np.uint32).tolist() == counts
    res = rep.tail_scores(h, permille=E2E["pm"])  # threshold=None: the reporter's relative one
    assert res.threshold_bucket.tolist() == T
    assert res.tail_ns.tolist() == [r["tail_ns"] for r in rows]
    assert res.total_ns.tolist() == [r["total_ns"] for r in rows]
    assert [REF.bits(s) for s in res.score] == [REF.bits(r["score"]) for r in rows]
    assert REF.bits(res.fleet_share) == REF.bits(float(sums[0]) / float(sums[1]))
    assert res.tail_calls is None
    # the tail score finds the rank ...
    assert np.nonzero(res.stragglers)[0].tolist() == [slow]
    assert res.score[slow] < 0.8 and all(res.score[r] > 1.0 for r in range(R) if r != slow)
    # ... that the report's median-based score does not see
    report = rep.report(ns, S)
    assert report.gpu_relative[slow] > E2E["thr"] and not report.stragglers_relative.any()
    # a second call reuses the reporter's buffers; tail_calls on request, on the device
    again = rep.tail_scores(h, permille=E2E["pm"], threshold=2.0, tail_calls=True)
    assert again.stragglers.tolist() == [True] * R
    assert [REF.bits(s) for s in again.score] == [REF.bits(r["score"]) for r in rows]
    assert again.tail_calls.is_cuda
    assert again.tail_calls.cpu().numpy().view(np.uint32).tolist() == [r["calls"] for r in rows]
    # and the report after it is the report before it
    report2 = rep.report(ns, S)
    assert np.array_equal(report2.gpu_relative, report.gpu_relative)


def test_matrix_reporter_rejects_bad_requests():
    rep = batch.MatrixReporter(2, 3, device=DEV)
    h = torch.zeros((2, 3, BINS), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="permille"):
        rep.tail_scores(h, permille=1001)
    with pytest.raises(ValueError, match="shape"):
        rep.tail_scores(h[:1])


# ---------------------------------------------------------------- one linear captured graph
def test_graph_capture_and_replay():
    R, K, pm, thr_s = 64, 67, 990, 0.9
    a, b = make_counts(R, K, seed=41), make_counts(R, K, seed=42)
    d = dev_counts(a).clone()
    fleet = torch.empty((K, BINS), dtype=torch.int64, device=DEV)
    thr = torch.empty(K, dtype=torch.int32, device=DEV)
    sums = torch.empty(2, dtype=torch.int64, device=DEV)
    out = ops.TailScores(torch.empty(R, dtype=torch.float64, device=DEV),
                         torch.empty(R, dtype=torch.int64, device=DEV),
                         torch.empty(R, dtype=torch.int64, device=DEV),
                         torch.empty(R, dtype=torch.uint8, device=DEV))
    calls = torch.empty((R, K), dtype=torch.int32, device=DEV)

    def three():
        ops.histogram_sum(d, out=fleet)
        ops.histogram_tail_threshold(fleet, pm, thr=thr, fleet_sums=sums)
        return ops.histogram_tail_scores(d, thr, sums, score_thr=thr_s, tail_calls=calls, out=out)

    three()  # the kernels are loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = three()
    for c in (b, a):  # two replays, the counts changed in between
        d.copy_(dev_counts(c))
        for t in (fleet, thr, sums, out.tail_ns, out.total_ns, calls):
            t.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        F, T, s, rows = REF.full(c.tolist(), pm, thr_s)
        assert u64_list(fleet.view(-1)) == [v for f in F for v in f]
        assert thr.cpu().tolist() == T and tuple(u64_list(sums)) == s
        assert_rows(res, rows, True)
