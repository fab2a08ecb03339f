"""CPU: the host twins of the compact history (``histograms.compact_*``,
``segment_compact_history_scores``).  Every case of ``_segment_history_cases`` is walked with the
compact twin in the three modes: the history stays canonical, N is the dense twin's, and where a
case never folds the compact history expands to exactly the dense twin's and every output is the
dense twin's bit for bit.  The fold rule is checked against a brute-force restatement in plain
dicts on the directed cases."""
import numpy as np
import pytest

import _compact_history_cases as C
import _segment_history_cases as H
from nvidia_resiliency_ext.straggler import histograms

FIELDS = ("score", "tail_ns", "total_ns", "base_tail_ns", "base_total_ns", "history_share",
          "stragglers", "threshold_bucket", "tail_calls")
MODES = (dict(update=False), dict(score=False), dict())


def dense_of(c, chist):
    """The dense expansion of the used slots of a case's history; the others zero."""
    used = C.used_slots(c)
    d = np.zeros(chist.shape[:2] + (C.BINS,), np.uint32)
    d[:, used] = histograms.compact_to_dense(chist[:, used])
    return d


def unused_untouched(c, chist):
    S = chist.shape[1]
    rest = sorted(set(range(S)) - set(C.used_slots(c)))
    return np.array_equal(chist[:, rest], c.chist0[:, rest])


def never_folds(name):
    """From the dense walk alone: no element of any history of the case has more than 12 buckets."""
    return all(int((res.hist != 0).sum(-1)[:, C.used_slots(C.case(name))].max(initial=0)) <= C.E
               for _, _, res in H.walk(name))


def test_thirteen_cases_never_fold_and_six_do():
    free = [c.name for c in H.cases() if never_folds(c.name)]
    assert len(free) >= 12 and len(H.cases()) - len(free) >= 5, free
    for c in C.converted():  # and the compact twin agrees on which they are
        folds = any(int(res.folded.sum()) for _, _, res in C.walk(c.name))
        assert folds != (c.name in free), c.name


@pytest.mark.parametrize("c", C.converted(), ids=lambda c: c.name)
def test_walk_against_the_dense_twin(c):
    free = never_folds(c.name)
    used = C.used_slots(c)
    for iv, (counts, h, fused), (dcounts, dh, dres) in zip(c.intervals, C.walk(c.name), H.walk(c.name)):
        assert np.array_equal(counts, dcounts)
        for kw in MODES:
            got = histograms.segment_compact_history_scores(
                iv.keys, iv.off, iv.lens, c.K, h, c.pm, iv.cap, score_thr=0.9, **kw,
                **C.history_kwargs(c))
            want = histograms.history_scores(dcounts, dh, c.pm, score_thr=0.9, **kw, **H.history_kwargs(c))
            assert histograms.compact_is_canonical(got.hist[:, used]).all()
            assert unused_untouched(c, got.hist)
            if kw.get("update", True):
                assert np.array_equal(got.hist, fused.hist) and np.array_equal(got.folded, fused.folded)
                # folding conserves N away from saturation
                n_c = dense_of(c, got.hist).astype(np.int64).sum(-1)
                n_d = want.hist.astype(np.int64).sum(-1)
                sat = (want.hist == 0xFFFFFFFF).any(-1) | (dense_of(c, got.hist) == 0xFFFFFFFF).any(-1)
                assert np.array_equal(n_c[:, used][~sat[:, used]], n_d[:, used][~sat[:, used]])
            else:
                assert np.array_equal(got.hist, h) and got.folded is None
            if free:
                assert np.array_equal(dense_of(c, got.hist)[:, used], want.hist[:, used])
                if kw.get("score", True):
                    for f in FIELDS:
                        assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), f
                if got.folded is not None:
                    assert not got.folded.any()


def brute_update(entries, samples):
    """The fold rule restated: entries {bucket: count}, samples a list of buckets."""
    c = {}
    for b in samples:
        c[b] = c.get(b, 0) + 1
    kept = set(entries)
    for b in sorted(c):
        if b not in kept and len(kept) < 12:
            kept.add(b)
    new, folded = {s: entries.get(s, 0) for s in kept}, 0
    for b, v in c.items():
        at_or_below = [s for s in kept if s <= b]
        t = max(at_or_below) if at_or_below else min(kept)
        new[t] += v
        folded += v if b not in kept else 0
    return {s: min(v, 2 ** 32 - 1) for s, v in new.items()}, folded


def entries_of(e):
    n = int(e[60:64].view("<u4")[0])
    return dict(zip(e[48:48 + n].tolist(), e[:4 * n].view("<u4").tolist()))


@pytest.mark.parametrize("c", C.directed(), ids=lambda c: c.name)
def test_fold_rule_against_a_brute_force_restatement(c):
    valid = [1] * c.K if c.col_valid is None else c.col_valid.tolist()
    skip = [0] * c.R if c.skip_rows is None else c.skip_rows.tolist()
    for iv, (counts, h, res) in zip(c.intervals, C.walk(c.name)):
        assert histograms.compact_is_canonical(res.hist).all()
        folded = [0] * c.R
        for r in range(c.R):
            for k in range(c.K):
                g = r * c.K + k
                n = int(iv.lens[g])
                keep = iv.cap if 0 < iv.cap < n else n
                e = int(iv.off[g]) + n
                samples = histograms.bucket_of(iv.keys[e - keep:e]).tolist() if n > 0 else []
                if not samples or not valid[k] or skip[r]:
                    assert np.array_equal(res.hist[r, k], h[r, k])
                    continue
                want, f = brute_update(entries_of(h[r, k]), samples)
                assert entries_of(res.hist[r, k]) == want, (r, k)
                folded[r] += f
        assert res.folded.tolist() == folded


def test_directed_cases_hit_what_they_aim_at():
    w = C.walk("fold_rule")
    e = [entries_of(w[0][2].hist[0, k]) for k in range(4)]
    assert e[0][120] == 5 + 3 and e[0][20] == 7 and 200 not in e[0]       # above all -> the highest
    assert e[1][10] == 5 + 4 and 3 not in e[1]                            # below all -> the lowest
    assert e[2][5] == 1 and e[2][20] == 4 and e[2][30] == 9 + 1 + 3 and e[2][50] == 9 + 2
    assert w[0][2].folded.tolist() == [3 + 4 + 3 + 2, 8 * 15]
    assert len(entries_of(w[0][2].hist[1, 0])) == 12
    assert entries_of(w[1][2].hist[0, 2])[5] == 1 + 2                      # bucket 0 -> the lowest, 5
    assert entries_of(w[0][2].hist[0, 3]) == {**C.FULL, 10: 12, 120: 6, 60: 35}
    assert not w[1][2].hist[1, 1].any()                                   # never a sample: empty
    s = C.walk("fold_saturates")
    assert entries_of(s[0][2].hist[0, 0])[50] == 2 ** 32 - 1 and entries_of(s[1][2].hist[0, 0])[50] == 2 ** 32 - 1
    assert [int(x[2].folded[0]) for x in s] == [1, 5]
    k = C.walk("skip_and_invalid")
    assert [x[2].folded.tolist() for x in k] == [[6, 0], [2, 0]]
    assert np.array_equal(k[1][2].hist[1], C.case("skip_and_invalid").chist0[1])
    f = C.walk("fused_fold_scores_before")
    assert f[0][2].tail_calls.tolist() == [[10]] and f[1][2].tail_calls.tolist() == [[10]]
    assert f[0][2].folded.tolist() == [10] and entries_of(f[0][2].hist[0, 0])[100] == 1060
    assert any(int(x[2].folded.sum()) for n in ("trips_unaligned", "compact_cap_trims") for x in C.walk(n))


def test_conversions():
    rng = np.random.default_rng(3)
    d = np.zeros((2, 3, 240), np.uint32)
    d[0, 0, [0, 7, 8, 239]] = [1, 2, 3, 2 ** 32 - 1]
    d[1, 2, rng.choice(240, 12, replace=False)] = rng.integers(1, 1000, 12)
    ch, folded = histograms.compact_from_dense(d)
    assert ch.shape == (2, 3, 64) and ch.dtype == np.uint8 and not folded.any()
    assert histograms.compact_is_canonical(ch).all() and not ch[0, 1].any()
    assert np.array_equal(histograms.compact_to_dense(ch), d)
    d[1, 1, 100:120] = 4  # 20 buckets: the 12 lowest kept, 8 x 4 samples folded into bucket 111
    ch, folded = histograms.compact_from_dense(d)
    assert folded.tolist() == [0, 32] and entries_of(ch[1, 1]) == {**{b: 4 for b in range(100, 111)}, 111: 36}
    bad = ch.copy()
    bad[0, 0, 48] = 9  # buckets no longer ascending
    assert histograms.compact_is_canonical(bad).tolist() == [[False, True, True], [True, True, True]]
    assert not histograms.compact_is_canonical(np.broadcast_to(C.SENTINEL, (1, 1, 64))).any()
    with pytest.raises(ValueError, match="canonical"):
        histograms.compact_to_dense(bad)
    with pytest.raises(ValueError, match="uint8"):
        histograms.compact_to_dense(np.zeros((1, 1, 60), np.uint8))
    with pytest.raises(ValueError, match="at least one"):
        histograms.compact_history_scores(d, ch, 990, score=False, update=False)
