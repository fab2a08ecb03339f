"""GPU: the individual tail-score kernels (nvrx_histogram_history_scores) against the definition in
plain Python integers (``_history_tail_ref``): integers equal, f64 bit patterns equal (NaN as NaN),
the history equal over its full tensor, no tolerance.  Every output is pre-filled with a sentinel.

The shapes sit on both sides of the split rule of DESIGN 3.12 (splits = min(ceil(2048 / R),
ceil(K / 16)), a split a whole number of 16-kernel trips): K <= 16 is one split; K = 67 is five
with a last split of 3 kernels; (2, 2049) and (1, 4100) are 129 and 257 splits with a last split of
1 and 4; (1024, 33) is limited by the 2,048-workgroup target (2 splits of 32 and 1).  K = 5, 67,
2049 are no multiple of waves x unroll = 16."""
import numpy as np
import pytest
import torch

import _history_tail_cases as C
import _history_tail_ref as HREF
from nvidia_resiliency_ext.straggler import ops

pytestmark = pytest.mark.gpu

BINS = 240
DEV = "cuda"
SENT = -7
BOTH = HREF.SCORE | HREF.UPDATE


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(DEV)


def u64_list(t):
    return t.cpu().numpy().view(np.uint64).tolist()


def sentinel_out(R):
    i = lambda: torch.full((R,), SENT, dtype=torch.int64, device=DEV)  # noqa: E731
    return ops.HistoryTailScores(torch.full((R,), float(SENT), dtype=torch.float64, device=DEV),
                                 i(), i(), i(), i(), torch.full((R,), 9, dtype=torch.uint8, device=DEV))


def run(c, h, pm, mode=BOTH, hist_index=None, hist_stride=0, col_valid=None, skip_rows=None,
        score_thr=0.9, calls=False, d_hist=None):
    """One call on fresh device copies; returns (result, the device history after the call, out)."""
    R, K = c.shape[:2]
    d_hist = dev(h) if d_hist is None else d_hist
    out = sentinel_out(R)
    t = lambda v, dt: None if v is None else torch.tensor(v, dtype=dt, device=DEV)  # noqa: E731
    tc = torch.full((R, K), SENT, dtype=torch.int32, device=DEV) if calls else False
    res = ops.histogram_history_scores(
        dev(c), d_hist, permille=pm, score=bool(mode & HREF.SCORE), update=bool(mode & HREF.UPDATE),
        hist_index=t(hist_index, torch.int32), hist_stride=hist_stride,
        col_valid=t(col_valid, torch.uint8), skip_rows=t(skip_rows, torch.uint8),
        score_thr=score_thr, tail_calls=tc, out=out)
    return res, d_hist, out


def assert_rows(res, rows, calls):
    for name in ("tail_ns", "total_ns", "base_tail_ns", "base_total_ns"):
        assert u64_list(getattr(res, name)) == [r[name] for r in rows], name
    assert [HREF.bits(s) for s in res.score.cpu().tolist()] == [HREF.bits(r["score"]) for r in rows]
    assert res.strag.cpu().tolist() == [int(r["strag"]) for r in rows]
    if calls:
        assert res.tail_calls.cpu().numpy().view(np.uint32).tolist() == [r["calls"] for r in rows]
    else:
        assert res.tail_calls is None


def assert_untouched(out):
    assert out.score.cpu().tolist() == [float(SENT)] * out.score.numel()
    for name in ("tail_ns", "total_ns", "base_tail_ns", "base_total_ns"):
        assert getattr(out, name).cpu().tolist() == [SENT] * out.score.numel(), name
    assert out.strag.cpu().tolist() == [9] * out.score.numel()


def hist_equal(d_hist, want):
    return np.array_equal(d_hist.cpu().numpy().view(np.uint32), want)


def check(c, h, pm, calls=False, **kw):
    """SCORE | UPDATE against the reference; returns the reference rows and new history."""
    ref_kw = {k: v for k, v in kw.items() if k != "hist_stride"}
    rows, new = C.reference(c, h, pm, BOTH, score_thr=0.9, **ref_kw)
    res, d_hist, _ = run(c, h, pm, calls=calls, **kw)
    assert_rows(res, rows, calls)
    assert hist_equal(d_hist, new)
    return rows, new


SHAPES = ([(R, K) for R in (1, 2, 3, 64, 257) for K in (1, 2, 5, 67)] +
          [(2, 2049), (1, 4100), (1024, 33)])
PMS = (990, 950, 500, 999)


@pytest.mark.parametrize("R,K", SHAPES)
def test_fused_call_equals_the_reference(R, K):
    i = SHAPES.index((R, K))
    c, h = C.random_case(R, K, seed=3000 + i)
    rows, _ = check(c, h, PMS[i % len(PMS)], calls=bool(i % 2))
    if R >= 3:
        assert rows[1]["score"] != rows[1]["score"] and not rows[1]["strag"]


@pytest.mark.parametrize("pm", (0, 500, 990, 1000))
@pytest.mark.parametrize("calls", (False, True))
def test_hand_made_cells(pm, calls):
    c, h, valid = C.hand_case()
    rows, new = check(c, h, pm, calls=calls, col_valid=valid)
    col = {n: i for i, n in enumerate(C.HAND)}
    T = rows[0]["T"]
    assert T[col["n1"]] == 100 and T[col["only239"]] == 239
    assert all(T[col[n]] == -1 for n in ("no_current", "no_history", "invalid"))
    if pm == 500:  # each of a lane's four bins, in lane 0 and in lane 59
        assert {n: T[col[n]] for n in C.HAND_T} == C.HAND_T
    k = col["topbit"]  # saturation
    assert new[0, k, 120] == C.FULL and new[0, k, 130] == C.FULL and new[0, k, 131] == C.TOP + 8
    assert np.array_equal(new[0, col["invalid"]], h[0, col["invalid"]])
    assert rows[1]["score"] != rows[1]["score"] and not new[1].any()  # the all-zero row


@pytest.mark.parametrize("R,K", [(3, 5), (64, 67)])
def test_col_valid_with_zeros(R, K):
    c, h = C.random_case(R, K, seed=8)
    valid = [int(k % 3 != 0) for k in range(K)]
    rows, new = check(c, h, 990, calls=True, col_valid=valid)
    assert np.array_equal(new[:, ::3], h[:, ::3])
    assert all(r["calls"][k] == 0 for r in rows for k in range(0, K, 3))


@pytest.mark.parametrize("R,K,S", [(3, 5, 9), (257, 67, 80)])
def test_hist_index_permutation_and_stride(R, K, S):
    c, h = C.random_case(R, K, seed=21, stride=S)
    rng = np.random.default_rng(22)
    h[:, K:] = rng.integers(0, 50, size=(R, S - K, BINS))
    # identity slots, stride > K: the slots beyond K are untouched
    _, new = check(c, h, 950, hist_stride=S)
    assert np.array_equal(new[:, K:], h[:, K:])
    # a permutation over all S slots with -1 entries
    index = rng.permutation(S)[:K].astype(np.int64)
    index[::4] = -1
    rows, new = check(c, h, 950, calls=True, hist_index=index.tolist(), hist_stride=S)
    free = sorted(set(range(S)) - {int(s) for s in index if s >= 0})
    assert np.array_equal(new[:, free], h[:, free])
    assert all(r["calls"][k] == 0 for r in rows for k in range(0, K, 4))


@pytest.mark.parametrize("R,K", [(3, 5), (64, 67)])
@pytest.mark.parametrize("calls", (False, True))
def test_mode_combinations(R, K, calls):
    c, h = C.random_case(R, K, seed=31)
    rows, new = C.reference(c, h, 990, BOTH, score_thr=0.9)
    # SCORE alone: the history is bit-identical afterwards
    res, d_hist, _ = run(c, h, 990, HREF.SCORE, calls=calls)
    assert_rows(res, rows, calls)
    assert hist_equal(d_hist, h)
    # UPDATE alone: the score outputs keep their sentinel
    res, d_hist, out = run(c, h, 990, HREF.UPDATE, calls=calls)
    assert hist_equal(d_hist, new)
    assert_untouched(out)
    assert res.tail_calls is None
    # both: the scores are from the history before the update
    res, d_hist, _ = run(c, h, 990, BOTH, calls=calls)
    assert_rows(res, rows, calls)
    assert hist_equal(d_hist, new)
    # skip_rows: scored, not absorbed
    skip = [int(r % 2) for r in range(R)]
    _, new_s = C.reference(c, h, 990, BOTH, skip_rows=skip)
    res, d_hist, _ = run(c, h, 990, BOTH, skip_rows=skip, calls=calls)
    assert_rows(res, rows, calls)
    assert hist_equal(d_hist, new_s) and np.array_equal(new_s[1], h[1])


def test_two_identical_calls_give_identical_bits():
    c, h = C.random_case(64, 67, seed=41)
    a, ha, _ = run(c, h, 990, calls=True)
    b, hb, _ = run(c, h, 990, calls=True)
    for name in ("score", "tail_ns", "total_ns", "base_tail_ns", "base_total_ns", "strag", "tail_calls"):
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), name
    assert torch.equal(ha, hb)


def intervals(R, K, n, seed):
    out = [C.random_case(R, K, seed=seed + i)[0] for i in range(n)]
    out[-1][0, :, 200] += 50  # the last interval of row 0 has a tail
    return out


def test_three_interval_sequence_equals_the_reference():
    R, K = 3, 21
    cs = intervals(R, K, 3, seed=51)
    h = np.zeros((R, K, BINS), np.uint32)
    d_hist = dev(h)
    for i, c in enumerate(cs):
        rows, h = C.reference(c, h, 990, BOTH, score_thr=0.9)
        res, d_hist, _ = run(c, None, 990, calls=True, d_hist=d_hist)
        assert_rows(res, rows, True)
        assert hist_equal(d_hist, h)
        if i == 0:  # no history yet: NaN, never flagged
            assert all(r["score"] != r["score"] and not r["strag"] for r in rows)


def test_graph_capture_and_replay():
    R, K, pm = 64, 67, 990
    ca, cb = intervals(R, K, 2, seed=61)
    _, h0 = C.random_case(R, K, seed=60)
    d = dev(ca).clone()
    d_hist = dev(h0).clone()
    out = sentinel_out(R)
    calls = torch.full((R, K), SENT, dtype=torch.int32, device=DEV)

    def fused():
        return ops.histogram_history_scores(d, d_hist, permille=pm, score_thr=0.9, tail_calls=calls,
                                            out=out)

    fused()  # the kernels are loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = fused()
    d_hist.copy_(dev(h0))
    h = h0
    for c in (ca, cb):  # two replays equal two eager calls: the second sees the first's history
        d.copy_(dev(c))
        for t in (out.tail_ns, out.total_ns, out.base_tail_ns, out.base_total_ns, calls):
            t.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        before = h
        rows, h = C.reference(c, before, pm, BOTH, score_thr=0.9)
        assert_rows(res, rows, True)
        assert hist_equal(d_hist, h)
        eager, e_hist, _ = run(c, before, pm, calls=True)
        assert torch.equal(eager.score.view(torch.int64), res.score.view(torch.int64))
        assert torch.equal(eager.tail_calls, res.tail_calls) and torch.equal(e_hist, d_hist)
