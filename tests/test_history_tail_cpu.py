"""CPU: ``histograms.history_scores``, the host twin of the individual tail scores, equals the
definition written in plain Python integers (``_history_tail_ref``) -- integers equal, f64 bit
patterns equal, the new history equal over its full array -- and the score behaves as the feature
promises on a rank that turns slow on every 16th call."""
import numpy as np
import pytest

import _history_tail_cases as C
import _history_tail_ref as HREF
from nvidia_resiliency_ext.straggler import histograms

PMS = (0, 500, 990, 1000)
MODES = {"score": HREF.SCORE, "update": HREF.UPDATE, "both": HREF.SCORE | HREF.UPDATE}


def check(c, h, pm, mode=HREF.SCORE | HREF.UPDATE, score_thr=0.9, **kw):
    rows, new = C.reference(c, h, pm, mode, score_thr=score_thr, **kw)
    h0 = h.copy()
    g = histograms.history_scores(c, h, pm, score=bool(mode & HREF.SCORE),
                                  update=bool(mode & HREF.UPDATE), score_thr=score_thr, **kw)
    assert np.array_equal(h, h0)  # the twin leaves its input alone
    assert g.hist.dtype == np.uint32 and np.array_equal(g.hist, new)
    if rows is None:
        assert g.score is None and g.tail_ns is None and g.tail_calls is None
        return g, rows
    for name in ("tail_ns", "total_ns", "base_tail_ns", "base_total_ns"):
        got = getattr(g, name)
        assert got.dtype == np.uint64 and got.tolist() == [r[name] for r in rows], name
    assert [HREF.bits(s) for s in g.score] == [HREF.bits(r["score"]) for r in rows]
    assert g.stragglers.tolist() == [r["strag"] for r in rows]
    assert g.tail_calls.tolist() == [r["calls"] for r in rows]
    assert g.threshold_bucket.tolist() == [r["T"] for r in rows]
    share = [float(r["base_tail_ns"]) / float(r["base_total_ns"]) if r["base_total_ns"] else float("nan")
             for r in rows]
    assert [HREF.bits(s) for s in g.history_share] == [HREF.bits(s) for s in share]
    return g, rows


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("pm", PMS)
@pytest.mark.parametrize("R,K", [(1, 1), (3, 5), (5, 19)])
def test_twin_equals_the_reference_on_random_cases(R, K, pm, mode):
    c, h = C.random_case(R, K, seed=100 * R + K)
    check(c, h, pm, MODES[mode])
    check(c.view(np.int32), h.view(np.int32), pm, MODES[mode])  # device arrays come as int32


@pytest.mark.parametrize("pm", PMS)
def test_hand_made_cells(pm):
    c, h, valid = C.hand_case()
    g, rows = check(c, h, pm, col_valid=valid)
    col = {n: i for i, n in enumerate(C.HAND)}
    T = rows[0]["T"]
    assert T[col["n1"]] == 100 and T[col["only239"]] == 239
    for n in ("no_current", "no_history", "invalid"):
        assert T[col[n]] == -1 and rows[0]["calls"][col[n]] == 0
    if pm == 500:
        assert {n: T[col[n]] for n in C.HAND_T} == C.HAND_T
    # saturation: 0x80000000 + 0xFFFFFFFF and 0xFFFFFFFF + 1 both stop at 2^32 - 1
    k = col["topbit"]
    assert g.hist[0, k, 120] == C.FULL and g.hist[0, k, 130] == C.FULL
    assert g.hist[0, k, 131] == C.TOP + 8 and g.hist[0, k, 132] == C.TOP
    # what is not taken keeps its history; the all-zero row scores NaN and is never flagged
    assert np.array_equal(g.hist[0, col["invalid"]], h[0, col["invalid"]])
    assert np.array_equal(g.hist[0, col["no_history"]], c[0, col["no_history"]])
    assert rows[1]["score"] != rows[1]["score"] and not rows[1]["strag"]
    assert not g.hist[1].any()


def test_hist_index_stride_and_skip_rows():
    R, K, S = 4, 9, 14
    c, h = C.random_case(R, K, seed=5, stride=S)
    rng = np.random.default_rng(6)
    h[:, K:] = rng.integers(0, 50, size=(R, S - K, C.BINS))
    index = rng.permutation(S)[:K].astype(np.int32)
    index[::4] = -1
    skip = [0, 1, 0, 1]
    g, rows = check(c, h, 950, hist_index=index.tolist(), skip_rows=skip)
    untouched = sorted(set(range(S)) - {int(s) for s in index if s >= 0})
    assert np.array_equal(g.hist[:, untouched], h[:, untouched])
    assert np.array_equal(g.hist[1], h[1]) and np.array_equal(g.hist[3], h[3])
    assert not np.array_equal(g.hist[0], h[0])
    assert all(r["calls"][k] == 0 for r in rows for k in range(0, K, 4))


def test_bad_requests():
    c, h = C.random_case(2, 3, seed=1)
    with pytest.raises(ValueError, match="permille"):
        histograms.history_scores(c, h, 1001)
    with pytest.raises(ValueError, match="at least one"):
        histograms.history_scores(c, h, 990, score=False, update=False)
    with pytest.raises(ValueError, match="shape"):
        histograms.history_scores(c, h[:1], 990)
    with pytest.raises(ValueError, match="hist_index"):
        histograms.history_scores(c, h, 990, hist_index=[0, 1, 3])


# ---------------------------------------------------------------- the scenario of the feature
KERNELS, CALLS, INTERVALS, FIRST_SLOW = 16, 256, 8, 5  # 0-based: intervals 5, 6, 7 are degraded


def interval_counts(rng, every):
    """[1, 16, 240] counts of one interval: 2 % jitter about a per-kernel base; `every` > 0 makes
    every `every`-th call 2x slower."""
    c = np.zeros((1, KERNELS, C.BINS), np.uint32)
    for k in range(KERNELS):
        d = (15_000 * (k + 2) * (1.0 + 0.02 * rng.random(CALLS))).astype(np.uint64)
        if every:
            d[::every] *= 2
        c[0, k] = np.bincount(histograms.bucket_of(d), minlength=C.BINS)
    return c


def run_scenario(pm, every, seed=77):
    """absorb="healthy" emulated: a score call, then an update call that skips the flagged row."""
    rng = np.random.default_rng(seed)
    hist = np.zeros((1, KERNELS, C.BINS), np.uint32)
    scores = []
    for i in range(INTERVALS):
        c = interval_counts(rng, every if i >= FIRST_SLOW else 0)
        s = histograms.history_scores(c, hist, pm, update=False, score_thr=0.95)
        hist = histograms.history_scores(c, hist, pm, score=False, skip_rows=s.stragglers).hist
        scores.append((float(s.score[0]), bool(s.stragglers[0])))
    return scores


@pytest.mark.parametrize("pm,every", [(990, 16), (950, 8)])
def test_scenario_rank_turns_slow_on_every_nth_call(pm, every):
    scores = run_scenario(pm, every)
    assert scores[0][0] != scores[0][0] and not scores[0][1]  # no history yet: NaN, not flagged
    for s, flag in scores[1:FIRST_SLOW]:
        assert abs(s - 1.0) < 0.01 and not flag
    # flagged intervals are not absorbed: the history stays healthy and every degraded interval
    # scores about 1 - (time lost), far below the healthy ones
    for s, flag in scores[FIRST_SLOW:]:
        assert s < 0.9 and flag


def test_scenario_nothing_injected():
    scores = run_scenario(990, 0)
    assert scores[0][0] != scores[0][0]
    assert all(abs(s - 1.0) < 0.01 and not flag for s, flag in scores[1:])
