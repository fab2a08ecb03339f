"""GPU: score attribution (csrc/attribution.hip) with the winners placed by the kernel's layout.

The reference and the comparison are those of tests/test_gpu_attribution.py: `expect` (float64
numpy, one rounding per operation, stable sort), idx / loss / score bit for bit, wsum against
math.fsum at 1e-12.  What is new is where the large losses sit.  Column k belongs to thread
k % 256 (wave k % 256 // 64); a thread's j-th batch is the columns tid + 256 (8 j + c), c < 8.  The
first batch inserts with the FIRST shortcut, the later ones with the general insertion, so K = 6149
(3 * 2048 + 5) gives every thread three batches of 8 columns and threads 0..4 one column of a
fourth.

The losses are exact by construction: num = 1, reference / history 1, MED 2, so s = 0.5 and
loss = AVG / 2, and AVG is a small integer (or the special value a case names): the order of the
losses is the order of AVG, and every case also states the winners it expects outright."""
import numpy as np
import pytest

from _score_ref import inputs
from test_gpu_attribution import check, run, same_bits

pytestmark = pytest.mark.gpu
K3 = 6149
TOPS = (1, 3, 4, 5, 8, 11, 16)
DTS = [np.float32, np.float64]
KINDS = ("relative", "individual")


def background(R, K, dt, seed):
    """Losses 0.5 .. 499.5 everywhere (ties among them): below every placed winner (>= 1000)."""
    g = np.random.default_rng(seed)
    return (np.ones((R, K), np.int32), np.full((R, K), 2.0, dt),
            g.integers(1, 1000, (R, K)).astype(dt))


def base_of(kind, R, K, dt):
    return dict(ref=np.ones(K, np.float32)) if kind == "relative" else dict(hist=np.ones((R, K), dt))


def check_all(num, med, avg, want_order=None, tops=TOPS, kinds=KINDS, **kw):
    """Every top and kind; want_order[r]: the columns of row r's placed winners, best first (the
    background follows where a row places fewer than top)."""
    R, K = med.shape
    for kind in kinds:
        for top in tops:
            gi, gl, gs, _ = check(num, med, avg, top=top, kind=kind, **base_of(kind, R, K, med.dtype), **kw)
            if want_order is not None:
                for r, order in enumerate(want_order):
                    assert gi[r, :len(order)].tolist() == list(order[:top]), (kind, top, r)


def thread_cols(t, K=K3, batches=3):
    return np.arange(t, K, 256)[:8 * batches]


# ------------------------------------------------------------------ (a)
@pytest.mark.parametrize("t", [0, 63, 64, 255])
@pytest.mark.parametrize("dt", DTS)
def test_all_winners_in_one_thread(dt, t):
    """The 24 columns of thread t are the row's 24 largest: increasing with the column (every
    insertion goes to the front and shifts the list), decreasing (insertions at the back, then the
    wave-wide skip), in random order.  The thread drops candidates and is popped `top` times."""
    num, med, avg = background(3, K3, dt, seed=t)
    cols = thread_cols(t)
    assert cols.size == 24
    g = np.random.default_rng(100 + t)
    vals = [2000 + np.arange(24), 2000 + np.arange(24)[::-1], 2000 + g.permutation(24)]
    for r in range(3):
        avg[r, cols] = vals[r]
    order = [cols[np.argsort(-v, kind="stable")] for v in vals]
    check_all(num, med, avg, order)


# ------------------------------------------------------------------ (b), (i)
def alternating(dt):
    """Rank j's winner in wave j % 4 (row 0), (3 j) % 4 (row 1), both with the lanes swapped
    (row 2: 3 j again, lane 63 first); lanes 0 and 63; the j-th winner in the thread's j-th column,
    so the 16 span all three batches."""
    num, med, avg = background(3, K3, dt, seed=21)
    order = []
    for r, (step, flip) in enumerate(((1, 0), (3, 0), (3, 1))):
        cols = [((step * j) % 4) * 64 + (63 if (j + flip) & 1 else 0) + 256 * j for j in range(16)]
        avg[r, cols] = 5000 - np.arange(16)
        order.append(cols)
    return num, med, avg, order


@pytest.mark.parametrize("dt", DTS)
def test_winners_alternate_between_waves(dt):
    num, med, avg, order = alternating(dt)
    waves = [[c % 256 // 64 for c in o] for o in order]
    assert waves[0] == [0, 1, 2, 3] * 4 and waves[1] == [0, 3, 2, 1] * 4
    assert all(a != b for w in waves for a, b in zip(w, w[1:]))  # a different wave every round
    check_all(num, med, avg, order)


@pytest.mark.parametrize("dt", DTS)
def test_alternating_winners_twice_identical(dt):
    num, med, avg, _ = alternating(dt)
    for kind in KINDS:
        kw = dict(top=16, kind=kind, **base_of(kind, 3, K3, dt))
        a, b = run(num, med, avg, **kw), run(num, med, avg, **kw)
        assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2])
        assert np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64))


# ------------------------------------------------------------------ (c)
@pytest.mark.parametrize("dt", DTS)
def test_ties_across_batches_threads_and_waves(dt):
    num, med, avg = background(2, K3, dt, seed=31)
    b = 256 * 8  # one batch further in the same thread
    groups = [(3000, [70, 70 + b, 70 + 2 * b]),            # batches 0, 1, 2 of thread 70
              (2900, [40 + b, 3 + 2 * b]),                 # threads 40 and 3 of wave 0
              (2800, [200, 10 + b, 100 + 2 * b])]          # waves 3, 0, 1
    want0 = []
    for v, cols in groups:
        avg[0, cols] = v
        want0 += sorted(cols)
    # 20 columns tie for first place over all four waves and all three batches
    tied = sorted(64 * (i % 4) + 3 * (i // 4) + 256 * (7 * i % 24) for i in range(20))
    assert len(set(tied)) == 20 and {c % 256 // 64 for c in tied} == {0, 1, 2, 3}
    avg[1, tied] = 4000
    check_all(num, med, avg, [want0, tied])


# ------------------------------------------------------------------ (d)
@pytest.mark.parametrize("dt", DTS)
def test_empty_threads_beside_full_ones(dt):
    """col_valid removes every column of lanes 1..62 of wave 1: their heads stay (key 0, NO_COL)
    through the wave-wide skip and wave_best, next to lanes 0 and 63, which hold the winners."""
    num, med, avg = background(3, K3, dt, seed=41)
    valid = np.ones(K3, np.uint8)
    lanes = np.arange(K3) % 256
    valid[(lanes > 64) & (lanes < 127)] = 0
    c64, c127 = thread_cols(64), thread_cols(127)
    avg[0, c64] = 2000 + np.arange(24)                     # everything in lane 0 of wave 1
    avg[1, c127] = 3000 - np.arange(24)                    # in lane 63
    avg[2, c64[::2]], avg[2, c127[1::2]] = 2500 - np.arange(12), 2600 - np.arange(12)
    avg[:, 65:K3:256] = 9000                               # the best losses sit in a removed thread
    order = [c64[::-1], c127, np.concatenate([c127[1::2], c64[::2]])]
    check_all(num, med, avg, order, col_valid=valid)
    # wave 1 alone: every other column removed as well, fewer candidates than top
    valid[:] = 0
    valid[c64[:3]] = valid[c127[:2]] = 1
    check_all(num, med, avg, tops=(8, 16), col_valid=valid)


# ------------------------------------------------------------------ (e)
@pytest.mark.parametrize("dt", DTS)
def test_winners_only_in_the_general_insertion_batches(dt):
    """Row 0: every column below 2048 (the FIRST batches) loses to every column from 2048 on;
    row 1: the reverse; row 2: the best 16 alternate between the two."""
    g = np.random.default_rng(51)
    num, med, avg = background(3, K3, dt, seed=51)
    late = np.arange(K3) >= 2048
    avg[0, late] += 1000
    avg[1, ~late] += 1000
    pick = np.stack([g.choice(2048, 8, replace=False), 2048 + g.choice(K3 - 2048, 8, replace=False)], 1).reshape(-1)
    avg[2, pick] = 7000 - np.arange(16)
    for kind in KINDS:
        for top in TOPS:
            gi, *_ = check(num, med, avg, top=top, kind=kind, **base_of(kind, 3, K3, dt))
            assert (gi[0] >= 2048).all() and (gi[1] < 2048).all() and gi[2].tolist() == pick[:top].tolist()


# ------------------------------------------------------------------ (f)
@pytest.mark.parametrize("K", [2048, 2049, 2304, 4096, 4097, K3])
@pytest.mark.parametrize("dt", DTS)
def test_batch_edges_with_every_option(dt, K):
    for R in (1, 3):
        x = inputs(R, K, dt, seed=1000 * R + K)
        n, m, a = x["num"], x["med"], x["avg"]
        for top in TOPS:
            check(n, m, a, top=top, kind="relative", col_valid=x["col_valid"], ref=x["ref"],
                  ref_index=x["perm"], ref_missing=x["missing"])
            check(n, m, a, top=top, kind="individual", col_valid=x["col_valid"], hist=x["hist"],
                  hist_index=x["slot"], hist_stride=x["stride"])


# ------------------------------------------------------------------ (g)
@pytest.mark.parametrize("dt", DTS)
def test_non_finite_and_tiny_losses(dt):
    """+inf, -inf and subnormal losses of both signs sort where IEEE order puts them; a NaN loss
    is left out.  Rows 0 and 1: only the special columns are present, so all of them are among the
    top 16 (+inf in row 0, -inf in row 1: a row with both has no weight sum); row 2: +inf and the
    others among a full finite background."""
    tiny = float(np.finfo(dt).smallest_subnormal)
    spec = [(1e30, 2048 + 7), (6.0, 255), (8 * tiny, 4096 + 64), (2 * tiny, 64),
            (-2 * tiny, 2048 + 255), (-4 * tiny, 63), (-6.0, 4096 + 63), (-1e30, 0)]
    hi, lo, nan_col = 300, 2048, 6148
    num, med, avg = background(3, K3, dt, seed=61)
    num[:2, :] = 0
    for v, c in spec:
        avg[:, c] = v
        num[:2, c] = 1
    avg[0, hi] = avg[2, hi] = np.inf
    avg[1, lo] = -np.inf
    num[0, hi] = num[1, lo] = 1
    avg[:, nan_col], num[:2, nan_col] = np.nan, 1
    cols = [c for _, c in spec]
    for kind in KINDS:
        for top in TOPS:
            gi, gl, _, _ = check(num, med, avg, top=top, kind=kind, **base_of(kind, 3, K3, dt))
            assert gi[0].tolist() == ([hi] + cols + [-1] * 16)[:top]
            assert gi[1].tolist() == (cols + [lo] + [-1] * 16)[:top]
            assert gi[2, 0] == hi and not (gi == nan_col).any()
        assert gl[0, 0] == np.inf and gl[1, 8] == -np.inf
        assert gl[0, 3] == 4 * tiny and gl[0, 4] == tiny and gl[0, 5] == -tiny  # loss = AVG / 2


# ------------------------------------------------------------------ (h)
@pytest.mark.parametrize("dt", DTS)
def test_many_rows_distinct_winners(dt):
    """R = 300 rows of K = 513 (two columns for thread 0, one for the others), each row with its
    own winners; history rows of K + 5 values each holding another power of two, MED twice that:
    reading a neighbour's row changes the score."""
    R, K, stride = 300, 513, 518
    num, med, avg = background(R, K, dt, seed=71)
    rows = np.arange(R)
    win = np.stack([(7 * rows + 31 * j) % K for j in range(16)], 1)
    assert all(len(set(w)) == 16 for w in win.tolist())
    avg[rows[:, None], win] = 3000 - np.arange(16)
    scale = (2.0 ** (rows % 5)).astype(dt)
    hist = np.full((R, stride), 64.0, dt)
    hist[:, :K] = scale[:, None]
    for top in TOPS:
        gi, *_ = check(num, med, avg, top=top, kind="relative", ref=np.ones(K, np.float32))
        assert np.array_equal(gi, win[:, :top])
        gi, _, gs, _ = check(num, (2 * scale)[:, None] * np.ones((1, K), dt), avg, top=top, kind="individual",
                             hist=hist, hist_stride=stride)
        assert np.array_equal(gi, win[:, :top]) and (gs == 0.5).all()
