"""CPU: the host twins of the tail score attribution (``histograms.tail_attribution`` /
``history_attribution``) equal the plain reference of ``_tail_attr_ref`` bit for bit on every
output over the shared case list, and the attribution names the kernel that costs a rank its tail
score where the count of tail calls names a cheap, jittery one."""
import numpy as np
import pytest

import _tail_attr_cases as C
import _tail_attr_ref as REF
from nvidia_resiliency_ext.straggler import histograms

FIELDS = ("idx", "loss", "tail_ns", "total_ns", "tail_calls", "thr_bucket", "base_share", "loss_all")


def twin(case):
    if case["kind"] == "relative":
        return histograms.tail_attribution(case["counts"], case["pm"], case["top"],
                                           col_valid=case["col_valid"], fleet=case["fleet"],
                                           thr_index=case["thr_index"])
    return histograms.history_attribution(case["counts"], case["hist"], case["pm"], case["top"],
                                          hist_index=case["hist_index"], col_valid=case["col_valid"])


def reference(case):
    lst = lambda v: None if v is None else np.asarray(v).tolist()  # noqa: E731
    if case["kind"] == "relative":
        return REF.relative(case["counts"].tolist(), case["pm"], case["top"], lst(case["col_valid"]),
                            lst(case["fleet"]), lst(case["thr_index"]))
    return REF.individual(case["counts"].tolist(), case["hist"].tolist(), case["pm"], case["top"],
                          lst(case["hist_index"]), lst(case["col_valid"]))


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want, dtype=got.dtype).reshape(got.shape)
    if got.dtype == np.float64:
        got, want = got.view(np.uint64), want.view(np.uint64)
        nan = np.float64("nan").view(np.uint64)
        # every NaN is "not taken": compare it as one pattern
        got = np.where(np.isnan(got.view(np.float64)), nan, got)
        want = np.where(np.isnan(want.view(np.float64)), nan, want)
    assert np.array_equal(got, want), what


@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_twin_equals_the_plain_reference(case):
    got, want = twin(case), reference(case)
    for f in FIELDS:
        same_bits(getattr(got, f), want[f], f)


def test_the_case_list_reaches_its_branches():
    seen = {f: False for f in ("empty-slot", "negative-row", "nan-left-out", "beyond-2^53", "tie")}
    for case in C.CASES:
        a = twin(case)
        seen["empty-slot"] |= bool((a.idx == -1).any())
        seen["negative-row"] |= bool(((a.idx[:, 0] >= 0) & (a.loss[:, 0] < 0)).any())
        seen["beyond-2^53"] |= bool((a.total_ns > (1 << 53)).any())
        seen["tie"] |= bool(((a.idx[:, 1:] >= 0) & (a.loss[:, 1:] == a.loss[:, :-1])).any())
        c = case["counts"].astype(np.int64)
        only0 = (c[:, :, 0] > 0) & (c[:, :, 1:].sum(2) == 0)
        seen["nan-left-out"] |= bool((only0 & np.isnan(a.loss_all)).any())
    assert all(seen.values()), seen
    assert {c["top"] for c in C.CASES} >= {1, 4, 5, 8, 16}
    assert {c["counts"].shape[1] for c in C.CASES} >= {1, 15, 16, 17, 33, 2048, 2049}


def scenario():
    """8 ranks x 6 kernels; rank 5's kernel 3 (2 ms) is 2x slower on every 16th call."""
    bases = [5_000, 200_000, 200_000, 2_000_000, 200_000, 200_000]
    calls = [4096, 256, 256, 64, 256, 256]
    jitter = [0.10, 0.02, 0.02, 0.02, 0.02, 0.02]
    rng = np.random.default_rng(7)
    c = np.zeros((8, 6, 240), np.uint32)
    for r in range(8):
        for k in range(6):
            d = bases[k] * (1.0 + jitter[k] * rng.standard_normal(calls[k]))
            if r == 5 and k == 3:
                d[::16] *= 2
            c[r, k] = np.bincount(histograms.bucket_of(d.astype(np.uint32)), minlength=240)
    return c


def test_a_count_is_not_a_cost():
    c = scenario()
    s = histograms.tail_scores(c, 950)
    a = histograms.tail_attribution(c, 950, 6)
    assert int(np.argmin(s.score)) == 5 and s.score[5] < 0.97 and np.delete(s.score, 5).min() > 1.0
    assert int(np.argmax(s.tail_calls[5])) == 0       # by tail calls the cheap, jittery kernel leads
    assert a.idx[5, 0] == 3                           # by excess tail time the 2 ms kernel does
    assert a.loss[5, 0] >= 10 * max(a.loss[5, 1], 0.0)
    for r in range(8):
        if r != 5:
            assert not (a.loss_all[r] > a.loss[5, 0] / 10).any(), r
    # per row the taken tails add up to the score's tail_ns
    assert np.array_equal(a.tail_ns.sum(1), s.tail_ns)
    ref = REF.relative(c.tolist(), 950, 6)
    assert [round(v) for v in ref["loss_all"][5]] == [53156, 0, 186361, 12823751, -53107, 0]
    assert s.tail_calls[5].tolist() == [49, 0, 1, 4, 0, 0]


def test_argument_checks():
    c = np.zeros((1, 2, 240), np.uint32)
    for top in (0, 17, True, 1.5):
        with pytest.raises(ValueError, match="top"):
            histograms.tail_attribution(c, 950, top)
        with pytest.raises(ValueError, match="top"):
            histograms.history_attribution(c, c, 950, top)
    with pytest.raises(ValueError, match="permille"):
        histograms.tail_attribution(c, 1001, 4)
    with pytest.raises(ValueError, match="hist_index"):
        histograms.history_attribution(c, c, 950, 4, hist_index=[0, 2])
