"""GPU: ``ops.score_rank_attribution`` (nvrx_score_rank_attribution) against the host twin
``histograms.score_rank_attribution``.  Shapes come from the plan function, so that every gate of
the launch is hit on both sides: fewer rows than waves, one split (one kernel writes the outputs)
against several (partial lists plus the merge kernel), a ragged last split, a partial column tile,
several tiles, every TOP instantiation with a smaller request inside it, f32 and f64 statistics,
both kinds, and the grid bound that caps the splits.  Every comparison is equality: integers, and
f64 as bits."""
import numpy as np
import pytest
import torch

from _score_ref import inputs
from nvidia_resiliency_ext.straggler import histograms, ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN = float("nan")
ROWS = (1, 3, 5, 63, 64, 65, 257)
COLS = (1, 63, 65, 130)
TOPS = (1, 3, 4, 8, 9, 16)
FIELDS = ("idx", "loss", "score", "taken", "positive")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def stats(R, K, dt, seed):
    """``inputs`` plus what the attribution must leave out: NaN AVG here and there."""
    x = inputs(R, K, dt, seed)
    g = np.random.default_rng(seed + 1)
    x["avg"][g.random((R, K)) < 0.03] = np.nan
    return x


def base_of(x, kind, plain=False):
    K = x["med"].shape[1]
    if kind == "relative":
        return dict(ref=x["ref"]) if plain else dict(
            col_valid=x["col_valid"], ref=x["ref"], ref_index=x["perm"], ref_missing=x["missing"])
    return dict(hist=np.ascontiguousarray(x["hist"][:, :K])) if plain else dict(
        col_valid=x["col_valid"], hist=x["hist"], hist_index=x["slot"], hist_stride=x["stride"])


def same(out, ref, tag=None):
    got = {f: getattr(out, f).cpu().numpy() for f in FIELDS}
    for f in ("idx", "taken", "positive"):
        assert got[f].dtype == np.int32 and np.array_equal(got[f], getattr(ref, f)), (f, tag)
    for f in ("loss", "score"):
        want = getattr(ref, f)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got[f]), nan), (f, tag)
        assert np.array_equal(bits(got[f][~nan]), bits(want[~nan])), (f, tag)
    assert np.array_equal(got["idx"] < 0, np.isnan(got["loss"])), tag
    return got


def check(x, top, kind, rows=None, plain=False, d=None):
    """One call on host statistics ``x`` (``d``: their device copies) against the twin."""
    kw = base_of(x, kind, plain)
    d = d if d is not None else {k: dev(v) for k, v in x.items() if isinstance(v, np.ndarray)}
    names = dict(ref_index="perm", ref_missing="missing", hist_index="slot")
    dkw = {k: (v if not isinstance(v, np.ndarray) else
               dev(v) if plain and k == "hist" else d[names.get(k, k)]) for k, v in kw.items()}
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.score_rank_attribution(d["num"], d["med"], d["avg"], top=top, kind=kind, rows=dev(rows),
                                     err=err, **dkw)
    ref = histograms.score_rank_attribution(x["num"], x["med"], x["avg"], top, kind, rows=rows, **kw)
    tag = (x["med"].shape, str(x["med"].dtype), top, kind, rows is not None, plain)
    got = same(out, ref, tag)
    assert int(err.item()) == ref.err, tag
    if "hist" in dkw:  # read only
        assert np.array_equal(dkw["hist"].cpu().numpy().view(np.uint8), kw["hist"].view(np.uint8)), tag
    return ref, got


def test_the_shapes_sit_on_both_sides_of_every_gate():
    splits = {R: ops.rank_attribution_plan(R, 130, 8)[1] for R in ROWS}
    assert [splits[R] for R in ROWS] == [1, 1, 1, 1, 1, 2, 5]
    assert ops.rank_attribution_plan(257, 130, 8)[2] > 0 == ops.rank_attribution_plan(64, 130, 8)[2]
    assert 257 % -(-257 // 5) != 0  # the last of the five splits is ragged
    assert [ops.rank_attribution_plan(64, K, 8)[0] for K in COLS] == [1, 1, 2, 3]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["relative", "individual"])
def test_every_shape_against_the_twin(dt, kind):
    for R in ROWS:
        for K in COLS:
            x = stats(R, K, dt, seed=1000 * R + K)
            d = {k: dev(v) for k, v in x.items() if isinstance(v, np.ndarray)}
            rows = (np.random.default_rng(R + K).random(R) < 0.7).astype(np.uint8)
            for i, top in enumerate(TOPS):
                check(x, top, kind, rows=rows if i % 2 else None, d=d)
            check(x, 8, kind, plain=True, d=d)  # no filter, no index, history rows of K


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_zero_med_sets_err_and_is_left_out(dt):
    for R in (5, 257):  # one split, and five
        x = stats(R, 65, dt, seed=R)
        x["col_valid"][[7, 64]] = 1
        x["missing"][x["perm"][[7, 64]]] = 0
        x["ref"][x["perm"][[7, 64]]] = 0.5
        x["num"][:, [7, 64]] = 4
        x["avg"][:, [7, 64]] = 1.5
        for kind in ("relative", "individual"):
            ref, _ = check(x, 4, kind)
            assert ref.err == 0  # err untouched at 0
        x["med"][R - 1, 64] = 0.0  # the last row of the last split, the partial tile's last column
        rows = np.ones(R, np.uint8)
        for kind in ("relative", "individual"):
            ref, _ = check(x, 4, kind)
            assert ref.err == 1 and R - 1 not in ref.idx[64] and ref.taken[64] == R - 1
            # the error word is OR-ed: other bits stay
            err = torch.full((1,), 4, dtype=torch.int32, device=DEV)
            kw = {k: dev(v) if isinstance(v, np.ndarray) else v for k, v in base_of(x, kind).items()}
            ops.score_rank_attribution(dev(x["num"]), dev(x["med"]), dev(x["avg"]), top=4, kind=kind,
                                       err=err, **kw)
            assert int(err.item()) == 5
        rows[R - 1] = 0  # a row that is off reports nothing
        assert check(x, 4, "relative", rows=rows)[0].err == 0
        x["num"][R - 1, 64] = 0  # MED == 0 on an absent kernel: no error from this one
        assert check(x, 4, "relative")[0].err == 0


@pytest.mark.parametrize("R", (64, 257))  # one split, and five of 52 rows
@pytest.mark.parametrize("top", (4, 16))
def test_adversarial_columns(R, top):
    K = 70  # a full tile and a partial one
    last = R - 1
    num = np.full((R, K), 2, np.int32)
    med = np.full((R, K), 2.0, np.float32)
    avg = np.full((R, K), 3.0, np.float32)
    ref = np.ones(K, np.float32)                    # every loss 2 * 3 * (1 - 1/2) = 3: all equal
    hot = [last, R // 2 + 1, 6, 3, R // 4 + 2, 5]   # named out of order: the lower row must win
    med[hot, 1] = 4.0                               # equal maxima in different waves and splits
    med[np.arange(1, R, 3)[:20], 2] = 8.0           # more than `top` equal maxima, scattered
    num[:, 3] = 0
    num[last, 3] = 2                                # the only taken row is the last of the last split
    num[:, 4] = 0                                   # a whole column not taken
    ref[6] = np.nan                                 # ... and one without a reference
    med[:, 7] = 1.0                                 # s = 1: loss +0.0 ...
    avg[1::2, 7] = -3.0                             # ... and -0.0, mixed across waves and splits
    med[:, 8] = 0.5 + np.arange(R) / 4.0            # negative losses first, distinct, increasing
    for c, n in ((9, top - 1), (10, top), (11, top + 1)):
        num[:, c] = 0                               # exactly top - 1, top, top + 1 taken ...
        num[last - np.arange(n), c] = 2             # ... all in the last split
    med[:, 63] = 16.0                               # the tile's last lane, and the next tile's first
    med[:, 64] = 0.25
    med[:, 69] = 1.0 + np.arange(R)[::-1]           # the last column of the partial tile
    x = dict(num=num, med=med, avg=avg, ref=ref)
    ref_, got = check(x, top, "relative", plain=True)
    assert ref_.idx[0].tolist() == list(range(top)) and (ref_.loss[0] == 3.0).all()
    assert ref_.idx[1, :min(top, 6)].tolist() == sorted(hot)[:min(top, 6)]
    assert ref_.idx[2].tolist() == np.arange(1, R, 3)[:top].tolist()
    assert ref_.idx[3].tolist() == [last] + [-1] * (top - 1) and ref_.taken[3] == 1
    assert ref_.taken[4] == ref_.taken[6] == 0 and (ref_.idx[[4, 6]] == -1).all()
    assert ref_.idx[7].tolist() == list(range(top)) and ref_.positive[7] == 0
    assert np.array_equal(np.signbit(got["loss"][7]), np.arange(top) % 2 == 1)  # -0.0 stays -0.0
    assert (got["score"][7] == 1.0).all()
    assert ref_.idx[8, 0] == last and ref_.positive[8] == R - 3 and ref_.loss[8, -1] > 0
    assert ref_.taken[9:12].tolist() == [top - 1, top, top + 1]
    assert ref_.idx[9].tolist() == list(range(R - top + 1, R)) + [-1]
    assert ref_.idx[10].tolist() == list(range(R - top, R))
    assert ref_.idx[11].tolist() == list(range(R - top - 1, R - 1))
    assert ref_.idx[69, 0] == 0 and ref_.idx[63].tolist() == list(range(top))
    # every row off: nothing is taken anywhere
    off, _ = check(x, top, "relative", rows=np.zeros(R, np.uint8), plain=True)
    assert (off.idx == -1).all() and not off.taken.any() and not off.positive.any()
    # the hot rows off one by one: the next one moves up
    rows = np.ones(R, np.uint8)
    rows[[3, 5]] = 0
    assert check(x, top, "relative", rows=rows, plain=True)[0].idx[1, 0] == 6


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_unfused_path_gives_the_same(dt):
    for R, K, top in ((65, 63, 9), (257, 130, 16), (5, 65, 3)):
        x = stats(R, K, dt, seed=R + K)
        x["med"][R // 2, K // 2] = 0.0
        rows = (np.arange(R) % 5 != 2).astype(np.uint8)
        for kind in ("relative", "individual"):
            kw = base_of(x, kind)
            loss_all, _, _ = histograms.score_losses(x["num"], x["med"], x["avg"], kind, **kw)
            for rw in (None, rows):
                _, got = check(x, top, kind, rows=rw)
                un = ops.rank_attribution(dev(loss_all), top, rows=dev(rw))
                assert np.array_equal(un.idx.cpu().numpy(), got["idx"])
                assert np.array_equal(bits(un.loss.cpu().numpy()), bits(got["loss"]))
                assert np.array_equal(un.taken.cpu().numpy(), got["taken"])
                assert np.array_equal(un.positive.cpu().numpy(), got["positive"])


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("R,K", [(16, 16), (7, 13), (3, 1)])
def test_the_other_direction_lists_the_same_elements(dt, R, K):
    x = stats(R, K, dt, seed=7 * R + K)
    for kind in ("relative", "individual"):
        kw = {k: dev(v) if isinstance(v, np.ndarray) else v for k, v in base_of(x, kind).items()}
        n, m, a = dev(x["num"]), dev(x["med"]), dev(x["avg"])
        rowwise = ops.score_attribution(n, m, a, top=16, kind=kind, **kw)
        colwise = ops.score_rank_attribution(n, m, a, top=16, kind=kind, **kw)
        ri, rl, rs = (t.cpu().numpy().reshape(R, 16) for t in (rowwise.idx, rowwise.loss, rowwise.score))
        ci, cl, cs = (t.cpu().numpy() for t in (colwise.idx, colwise.loss, colwise.score))
        by_row = {(r, int(ri[r, j]), int(bits(rl[r, j:j + 1])[0]), int(bits(rs[r, j:j + 1])[0]))
                  for r in range(R) for j in range(16) if ri[r, j] >= 0}
        by_col = {(int(ci[k, j]), k, int(bits(cl[k, j:j + 1])[0]), int(bits(cs[k, j:j + 1])[0]))
                  for k in range(K) for j in range(16) if ci[k, j] >= 0}
        assert by_row == by_col and len(by_col) == int(colwise.taken.sum().item())


def test_two_calls_write_identical_bytes_whatever_the_work_space_held():
    R, K, top = 257, 130, 9
    x = stats(R, K, np.float32, seed=5)
    kw = base_of(x, "individual")
    d = {k: dev(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    n, m, a = dev(x["num"]), dev(x["med"]), dev(x["avg"])
    need = ops.rank_attribution_plan(R, K, top)[2]
    assert need > 0
    got = []
    for fill in (0xFF, 0x00):
        buf = torch.full((ops.ScoreRankAttribution.nbytes(K, top),), 0xA5, dtype=torch.uint8, device=DEV)
        work = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
        ops.score_rank_attribution(n, m, a, top=top, kind="individual", work=work,
                                   out=ops.ScoreRankAttribution.packed(buf, K, top), **d)
        got.append(buf.cpu().numpy())
    assert np.array_equal(got[0], got[1])
    idx, loss, score, taken, positive = ops.ScoreRankAttribution.unpack(got[0], K, top)
    ref = histograms.score_rank_attribution(x["num"], x["med"], x["avg"], top, "individual", **kw)
    assert np.array_equal(idx, ref.idx) and np.array_equal(taken, ref.taken)
    assert np.array_equal(positive, ref.positive)
    nan = np.isnan(ref.loss)
    assert np.array_equal(np.isnan(loss), nan) and np.array_equal(np.isnan(score), nan)
    assert np.array_equal(bits(loss[~nan]), bits(ref.loss[~nan]))
    assert np.array_equal(bits(score[~nan]), bits(ref.score[~nan]))


def test_the_grid_bound_caps_the_splits():
    # 65 rows ask for two splits; 2,048 column tiles leave room for one
    R, K, top = 65, 2047 * 64 + 1, 4
    assert ops.rank_attribution_plan(R, K, top) == (2048, 1, 0)
    assert ops.rank_attribution_plan(R, K - 1, top)[:2] == (2047, 2)
    g = np.random.default_rng(11)
    x = dict(num=g.integers(0, 3, (R, K)).astype(np.int32),
             med=g.integers(1, 5, (R, K)).astype(np.float32),
             avg=g.integers(1, 4, (R, K)).astype(np.float32),
             ref=g.integers(-1, 2, K).astype(np.float32))
    check(x, top, "relative", plain=True)


def test_refusals_allocate_nothing():
    R, K = 65, 4
    f = torch.ones((R, K), device=DEV)
    n = torch.ones((R, K), dtype=torch.int32, device=DEV)
    ref = torch.ones(K, device=DEV)
    u8 = lambda k: torch.ones(k, dtype=torch.uint8, device=DEV)  # noqa: E731
    small_out = ops.ScoreRankAttribution.empty(K, 3, DEV)
    bad = [
        (ValueError, "ref", dict(num=n, med=f, avg=f, top=2, kind="relative")),
        (ValueError, "hist", dict(num=n, med=f, avg=f, top=2, kind="individual")),
        (ValueError, "device", dict(num=n.cpu(), med=f, avg=f, top=2, kind="relative", ref=ref)),
        (TypeError, "dtype", dict(num=n, med=f, avg=f.double(), top=2, kind="relative", ref=ref)),
        (TypeError, "dtype", dict(num=n, med=f, avg=f, top=2, kind="individual", hist=f.double())),
        (TypeError, "int32", dict(num=n.long(), med=f, avg=f, top=2, kind="relative", ref=ref)),
        (ValueError, "shape", dict(num=n[:, :3], med=f, avg=f, top=2, kind="relative", ref=ref)),
        (ValueError, "contiguous", dict(num=n, med=f.t().contiguous().t(), avg=f, top=2,
                                        kind="relative", ref=ref)),
        (ValueError, "hist_stride", dict(num=n, med=f, avg=f, top=2, kind="individual", hist=f,
                                         hist_index=torch.zeros(K, dtype=torch.int32, device=DEV))),
        (ValueError, "rows", dict(num=n, med=f, avg=f, top=2, kind="relative", ref=ref, rows=u8(R - 1))),
        (ValueError, "work", dict(num=n, med=f, avg=f, top=2, kind="relative", ref=ref, work=u8(8))),
        (ValueError, "out.idx", dict(num=n, med=f, avg=f, top=2, kind="relative", ref=ref,
                                     out=small_out)),
        (ValueError, "top", dict(num=n, med=f, avg=f, top=17, kind="relative", ref=ref)),
        (ValueError, "kind", dict(num=n, med=f, avg=f, top=2, kind="tail", ref=ref)),
    ]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for exc, word, kw in bad:
        rest = {k: v for k, v in kw.items() if k not in ("num", "med", "avg")}
        with pytest.raises(exc, match=word):
            ops.score_rank_attribution(kw["num"], kw["med"], kw["avg"], **rest)
    assert torch.cuda.memory_allocated() == before  # (`bad` keeps every input alive)


def test_captured_in_a_graph():
    R, K, top = 257, 130, 8
    x = stats(R, K, np.float32, seed=21)
    x["med"][201, 129] = 0.0
    x["num"][201, 129] = 3
    x["col_valid"][129] = 1
    kw = {k: dev(v) if isinstance(v, np.ndarray) else v for k, v in base_of(x, "individual").items()}
    n, m, a = dev(x["num"]), dev(x["med"]), dev(x["avg"])
    rows = torch.from_numpy((np.arange(R) % 5 != 0).astype(np.uint8)).to(DEV)
    eager = ops.score_rank_attribution(n, m, a, top=top, kind="individual", rows=rows, **kw)
    buf = torch.zeros(ops.ScoreRankAttribution.nbytes(K, top), dtype=torch.uint8, device=DEV)
    out = ops.ScoreRankAttribution.packed(buf, K, top)
    work = torch.empty(ops.rank_attribution_plan(R, K, top)[2], dtype=torch.uint8, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.score_rank_attribution(n, m, a, top=top, kind="individual", rows=rows, err=err, out=out,
                                   work=work, **kw)
    for _ in range(2):
        buf.fill_(0x5A)
        err.zero_()
        g.replay()
        torch.cuda.synchronize()
        for name in ("idx", "taken", "positive"):
            assert torch.equal(getattr(out, name), getattr(eager, name)), name
        for name in ("loss", "score"):
            assert torch.equal(getattr(out, name).view(torch.int64),
                               getattr(eager, name).view(torch.int64)), name
        assert int(err.item()) == 1
    ref = histograms.score_rank_attribution(x["num"], x["med"], x["avg"], top, "individual",
                                            rows=rows.cpu().numpy(), **base_of(x, "individual"))
    assert ref.err == 1
    same(out, ref)
