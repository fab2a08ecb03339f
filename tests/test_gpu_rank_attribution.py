"""GPU: ``ops.rank_attribution`` (nvrx_rank_attribution) against the host twin
``histograms.rank_attribution``.  Shapes come from the plan function, so that every gate of the
launch is hit on both sides: fewer rows than waves, one split (one kernel writes the outputs)
against several (partial lists plus the merge kernel), a ragged last split, a partial column tile,
several tiles, a row stride above K, every TOP instantiation with a smaller request inside it, and
the grid bound that caps the splits.  Every comparison is equality: integers, and f64 as bits."""
import numpy as np
import pytest
import torch

from nvidia_resiliency_ext.straggler import histograms, ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN, INF = float("nan"), float("inf")
ROWS = (1, 3, 4, 5, 63, 64, 65, 257)
COLS = (1, 63, 64, 65, 130)
TOPS = (1, 3, 4, 5, 8, 9, 16)


def matrix(R, K, seed, nan=0.3):
    """Small integers (many ties), signed zeros, a few infinities and NaNs."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-4, 5, size=(R, K)).astype(np.float64)
    x[rng.random((R, K)) < 0.02] = INF
    x[rng.random((R, K)) < 0.02] = -INF
    z = x == 0.0
    x[z] = np.where(rng.random(int(z.sum())) < 0.5, -0.0, 0.0)
    x[rng.random((R, K)) < nan] = NAN
    return x


def device_result(x, top, rows=None, ld=None, **kw):
    R, K = x.shape
    if ld is None:
        t = torch.from_numpy(x).to(DEV)
    else:  # rows ld elements apart, the padding poisoned with values that would win
        full = torch.full((R, ld), 1e300, dtype=torch.float64, device=DEV)
        full[:, :K] = torch.from_numpy(x).to(DEV)
        t = full[:, :K]
    r = None if rows is None else torch.from_numpy(np.asarray(rows)).to(DEV)
    out = ops.rank_attribution(t, top, rows=r, **kw)
    torch.cuda.synchronize()
    return out


def check(x, top, rows=None, ld=None):
    out = device_result(x, top, rows, ld)
    ref = histograms.rank_attribution(x, top, rows)
    assert np.array_equal(out.idx.cpu().numpy(), ref.idx)
    assert np.array_equal(out.loss.cpu().numpy().view(np.uint64), ref.loss.view(np.uint64))
    assert np.array_equal(out.taken.cpu().numpy(), ref.taken)
    assert np.array_equal(out.positive.cpu().numpy(), ref.positive)
    return ref


def test_the_shapes_sit_on_both_sides_of_every_gate():
    splits = {R: ops.rank_attribution_plan(R, 130, 8)[1] for R in ROWS}
    assert [splits[R] for R in ROWS] == [1, 1, 1, 1, 1, 1, 2, 5]
    assert ops.rank_attribution_plan(257, 130, 8)[2] > 0 == ops.rank_attribution_plan(64, 130, 8)[2]
    assert 257 % -(-257 // 5) != 0  # the last of the five splits is ragged
    assert [ops.rank_attribution_plan(64, K, 8)[0] for K in COLS] == [1, 1, 1, 2, 3]


@pytest.mark.parametrize("top", TOPS)
def test_every_shape_against_the_twin(top):
    for R in ROWS:
        for K in COLS:
            x = matrix(R, K, seed=1000 * R + K)
            check(x, top)
            rows = np.random.default_rng(R + K).random(R) < 0.7
            check(x, top, rows=rows.astype(np.uint8))


@pytest.mark.parametrize("top", (3, 16))
def test_row_stride_above_K(top):
    for R, K, ld in ((5, 63, 64), (65, 65, 70), (257, 130, 131)):
        check(matrix(R, K, seed=R), top, ld=ld)
        check(matrix(R, K, seed=R + 1), top, rows=np.arange(R) % 3 != 0, ld=ld)


@pytest.mark.parametrize("R", (64, 257))  # one split, and five of 52 rows
@pytest.mark.parametrize("top", (4, 16))
def test_adversarial_columns(R, top):
    K = 70  # a full tile and a partial one
    x = np.full((R, K), NAN)
    last = R - 1
    x[:, 0] = 2.5                                   # all equal: rows 0..top-1
    x[:, 1] = -1.0                                  # equal maxima in different waves and splits,
    hot = [last, R // 2 + 1, 6, 3, R // 4 + 2, 5]   # named out of order: the lower row must win
    x[hot, 1] = 7.0
    x[:, 2] = 1.0                                   # more than `top` equal maxima, scattered
    x[np.arange(1, R, 3)[:20], 2] = 9.0
    x[last, 3] = -3.0                               # the only taken row is the last of the last split
    x[:, 5] = np.arange(R)                          # NaN-only columns 4 and 6 next to full ones
    x[:, 7] = -np.arange(R, dtype=np.float64)       # -0.0 in row 0 is the maximum
    x[:, 63] = INF                                  # the tile's last lane, and the next tile's first
    x[:, 64] = -INF
    x[::2, 65] = 0.0                                # signed zeros tie across waves and splits
    x[1::2, 65] = -0.0
    x[:, 69] = np.arange(R)[::-1]                   # the last column of the partial tile
    ref = check(x, top)
    assert ref.idx[0].tolist() == list(range(top))
    assert ref.idx[1, :min(top, 6)].tolist() == sorted(hot)[:min(top, 6)]
    assert ref.idx[2].tolist() == np.arange(1, R, 3)[:top].tolist()
    assert ref.idx[3].tolist() == [last] + [-1] * (top - 1) and ref.taken[3] == 1
    assert ref.taken[4] == ref.taken[6] == 0 and ref.idx[5, 0] == last
    assert ref.idx[65].tolist() == list(range(top)) and ref.positive[65] == 0
    # every row off: nothing is taken anywhere
    off = check(x, top, rows=np.zeros(R, np.uint8))
    assert (off.idx == -1).all() and not off.taken.any() and not off.positive.any()
    # the hot rows off one by one: the next one moves up
    rows = np.ones(R, np.uint8)
    rows[[3, 5]] = 0
    assert check(x, top, rows=rows).idx[1, 0] == 6


def test_two_calls_write_identical_bytes_whatever_the_work_space_held():
    R, K, top = 257, 130, 9
    x = matrix(R, K, seed=5)
    t = torch.from_numpy(x).to(DEV)
    need = ops.rank_attribution_plan(R, K, top)[2]
    assert need > 0
    got = []
    for fill in (0x00, 0xFF):
        buf = torch.full((ops.RankAttribution.nbytes(K, top),), 0xA5, dtype=torch.uint8, device=DEV)
        work = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
        ops.rank_attribution(t, top, out=ops.RankAttribution.packed(buf, K, top), work=work)
        got.append(buf.cpu().numpy())
    assert np.array_equal(got[0], got[1])
    idx, loss, taken, positive = ops.RankAttribution.unpack(got[0], K, top)
    ref = histograms.rank_attribution(x, top)
    assert np.array_equal(idx, ref.idx) and np.array_equal(loss.view(np.uint64), ref.loss.view(np.uint64))
    assert np.array_equal(taken, ref.taken) and np.array_equal(positive, ref.positive)


def test_the_grid_bound_caps_the_splits():
    # 65 rows ask for two splits; 2,048 column tiles leave room for one
    R, K, top = 65, 2047 * 64 + 1, 4
    assert ops.rank_attribution_plan(R, K, top) == (2048, 1, 0)
    assert ops.rank_attribution_plan(R, K - 1, top)[:2] == (2047, 2)
    check(matrix(R, K, seed=11, nan=0.5), top)


def test_refusals():
    x = torch.zeros((4, 4), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="device"):
        ops.rank_attribution(x.cpu(), 2)
    with pytest.raises(ValueError, match="float64"):
        ops.rank_attribution(x.float(), 2)
    with pytest.raises(ValueError, match="float64"):
        ops.rank_attribution(x[0], 2)
    with pytest.raises(ValueError, match="contiguous rows"):
        ops.rank_attribution(x.t(), 2)
    with pytest.raises(ValueError, match="rows"):
        ops.rank_attribution(x, 2, rows=torch.ones(3, dtype=torch.uint8, device=DEV))
    big = torch.zeros((65, 4), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="work"):
        ops.rank_attribution(big, 2, work=torch.empty(8, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="out.idx"):
        ops.rank_attribution(x, 2, out=ops.RankAttribution.empty(4, 3, DEV))


def test_captured_in_a_graph():
    R, K, top = 257, 130, 8
    x = matrix(R, K, seed=21)
    t = torch.from_numpy(x).to(DEV)
    rows = torch.from_numpy((np.arange(R) % 5 != 0).astype(np.uint8)).to(DEV)
    eager = ops.rank_attribution(t, top, rows=rows)
    buf = torch.zeros(ops.RankAttribution.nbytes(K, top), dtype=torch.uint8, device=DEV)
    out = ops.RankAttribution.packed(buf, K, top)
    work = torch.empty(ops.rank_attribution_plan(R, K, top)[2], dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.rank_attribution(t, top, rows=rows, out=out, work=work)
    for _ in range(2):
        buf.fill_(0x5A)
        g.replay()
        torch.cuda.synchronize()
        for name in ("idx", "taken", "positive"):
            assert torch.equal(getattr(out, name), getattr(eager, name)), name
        assert torch.equal(out.loss.view(torch.int64), eager.loss.view(torch.int64))
    ref = histograms.rank_attribution(x, top, rows.cpu().numpy())
    assert np.array_equal(out.idx.cpu().numpy(), ref.idx)
