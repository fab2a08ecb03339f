"""GPU: ops.scores, ops.kernel_ref, ops.finalize_scores, ops.stragglers and ops.pack_min_times
against the plain float64 reference of tests/_score_ref.py.

Tolerance (derived, not tuned).  Every per-element term is a separately rounded float64
operation, so kernel and reference hold the same n non-negative terms t_k (and weights w_k) bit
for bit; only the order of the additions differs.  Adding n non-negative float64 numbers in any
order makes n - 1 roundings, each at most 2^-53 relative to a partial sum that is itself at most
the total, so to first order |sum - exact| <= (n - 1) * 2^-53 * exact; the reference's math.fsum
is the exact sum rounded once (another 2^-53).  Hence
    |S_gpu - fsum| <= n * 2^-53 * fsum                    for S = sum t and S = sum w,
n itself is exact, and the score sum t / sum w carries the two sums' errors and one rounding of
the division on each side:
    |score_gpu - score_ref| <= (2n + 2) * 2^-53 * score_ref.
With round_f32 the reference is rounded to float32 and bits are equal, except where the float64
reference lies within that bound of a float32 rounding boundary: there either neighbour passes.
Nothing in this file is looser.  Masks, counts, error bits and the history are exact; so is
everything about finalize_scores (the ABI fixes its order), kernel_ref, stragglers and
pack_min_times."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _score_ref as R
import oracle as O
from nvidia_resiliency_ext.straggler import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
KS = [1, 2, 255, 256, 257, 2047, 2048, 2049, 4097]
INF_BITS = 0x7F800000


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.cpu().numpy()


def forms(x):
    """The four argument forms of one input set: name -> the keyword arrays (numpy)."""
    K = x["med"].shape[1]
    rel = dict(col_valid=x["col_valid"], ref=x["ref"], ref_index=x["perm"], ref_missing=x["missing"])
    ind = dict(col_valid=x["col_valid"], hist=x["hist"], hist_index=x["slot"], hist_stride=x["stride"])
    plain = dict(ref=x["ref"], hist=np.ascontiguousarray(x["hist"][:, :K]))
    return dict(rel=rel, ind=ind, both={**rel, **ind}, plain=plain)


def run(x, kw, *, path="partials", round_f32=False, thr_rel=0.75, thr_ind=0.75, err0=0, hist=None,
        **extra):
    """One ops.scores call on host arrays, finished through finalize_scores ("partials") or in
    the kernel ("fused").  hist: a device history to keep using instead of a fresh upload."""
    Rr = x["med"].shape[0]
    d = {k: dev(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    if hist is not None:
        d["hist"] = hist
    err = torch.full((1,), err0, dtype=torch.int32, device=DEV)
    num, med, avg = dev(x["num"]), dev(x["med"]), dev(x["avg"])
    if path == "partials":
        p = ops.scores(num, med, avg, err=err, **d, **extra)
        gr, gi, mr, mi = ops.finalize_scores(p, Rr, 1, round_f32, thr_rel, thr_ind, err=err)
    else:
        p = torch.empty((Rr, 6), dtype=torch.float64, device=DEV)
        gr, gi = (torch.empty(Rr, dtype=torch.float64, device=DEV) for _ in range(2))
        mr, mi = (torch.empty(Rr, dtype=torch.uint8, device=DEV) for _ in range(2))
        fz = dict(gpu_rel=gr, gpu_ind=gi, strag_rel=mr, strag_ind=mi, thr_rel=thr_rel,
                  thr_ind=thr_ind, round_f32=round_f32)
        ops.scores(num, med, avg, partials=p, err=err, finalize=fz, **d, **extra)
    return SimpleNamespace(p=host(p), sr=host(gr), si=host(gi), mr=host(mr), mi=host(mi),
                           err=int(err.item()), hist=host(d.get("hist")), dhist=d.get("hist"))


def check_score(got, want, n, thr, got_mask, round_f32):
    nan = n == 0
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(want), nan)
    g, w, b = got[~nan], want[~nan], R.score_rel_bound(n[~nan])
    with np.errstate(all="ignore"):
        print("score rel err / bound:", (np.abs(g - w) / (b * np.abs(w))).max() if len(g) else None)
    assert (np.abs(w - thr) > b * np.abs(w)).all()  # the inputs keep the mask unambiguous
    if round_f32:
        lo, hi = (w * (1 - b)).astype(np.float32), (w * (1 + b)).astype(np.float32)
        g32 = g.astype(np.float32)
        assert np.array_equal(g32.astype(np.float64), g)  # a float32 value
        assert ((g32 == lo) | (g32 == hi)).all()  # lo == hi away from a rounding boundary: bits
        w = w.astype(np.float32).astype(np.float64)
    else:
        assert (np.abs(g - w) <= b * np.abs(w)).all()
    assert got_mask.dtype == np.uint8 and set(np.unique(got_mask)) <= {0, 1}
    assert np.array_equal(got_mask.astype(bool), R.stragglers(got, thr))  # follows the value stored
    want_mask = np.zeros(len(n), bool)
    want_mask[~nan] = w < thr
    assert np.array_equal(got_mask.astype(bool), want_mask)


def check(got, want, *, round_f32=False, thr_rel=0.75, thr_ind=0.75):
    p = want.partials
    assert np.array_equal(got.p[:, [2, 5]], p[:, [2, 5]])  # n: exact
    for base in (0, 3):
        n = p[:, base + 2]
        for i in (base, base + 1):
            assert (np.abs(got.p[:, i] - p[:, i]) <= R.sum_bound(n, p[:, i])).all(), (base, i)
    sr, si, _, _, _ = R.finish(p)
    check_score(got.sr, sr, p[:, 2], thr_rel, got.mr, round_f32)
    check_score(got.si, si, p[:, 5], thr_ind, got.mi, round_f32)
    if want.new_hist is not None:  # every element of [R, stride], padding and filtered slots too
        assert R.same_bits(got.hist, want.new_hist)


def same_result(a, b):
    return (R.same_bits(a.p, b.p) and R.same_bits(a.sr, b.sr) and R.same_bits(a.si, b.si) and
            np.array_equal(a.mr, b.mr) and np.array_equal(a.mi, b.mi) and
            (a.hist is None or R.same_bits(a.hist, b.hist)))


# ------------------------------------------------------------------ scores: the option matrix
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_scores_option_matrix(dt, K):
    for rows in (1, 3):
        x = R.score_inputs(rows, K, dt, seed=1000 * rows + K)
        for name, kw in forms(x).items():
            want = R.score_terms(x["num"], x["med"], x["avg"], **kw)
            assert (want.w[want.elig] >= 0).all()
            a, b = run(x, kw, path="partials"), run(x, kw, path="fused")
            assert same_result(a, b), name  # the two ways to finish: bit for bit
            assert a.err == b.err == 0, name
            check(a, want)
            check(b, want)
            r32 = run(x, kw, path="fused", round_f32=True)
            check(r32, want, round_f32=True)


def test_history_update_every_slot_and_second_call():
    for dt in (np.float32, np.float64):
        x = R.score_inputs(3, 2049, dt, seed=77)
        kw = forms(x)["ind"]
        old = x["hist"][:, x["slot"]]
        elig = (x["num"] > 0) & (x["col_valid"] != 0)
        # the inputs hold every case: a stored value above / below MED, +inf, untouched slots
        assert (elig & (old > x["med"]) & np.isfinite(old)).any() and (elig & (old < x["med"])).any()
        assert (elig & np.isinf(old)).any() and (~elig & (old > x["med"])).any()
        want = R.score_terms(x["num"], x["med"], x["avg"], **kw)
        got = run(x, kw)
        check(got, want)
        pad = np.setdiff1d(np.arange(x["stride"]), x["slot"])
        assert R.same_bits(got.hist[:, pad], x["hist"][:, pad])
        keep = ~elig
        assert R.same_bits(got.hist[:, x["slot"]][keep], old[keep])
        # +inf everywhere: the first call stores MED, so the second scores exactly 1 per kernel
        kw = dict(kw, hist=np.full_like(x["hist"], np.inf))
        first = run(x, kw)
        second = run(x, kw, hist=first.dhist)
        want2 = R.score_terms(x["num"], x["med"], x["avg"], **dict(kw, hist=first.hist))
        check(second, want2)
        n, st, sw = second.p[:, 5], second.p[:, 3], second.p[:, 4]
        assert (np.abs(st - sw) <= R.sum_bound(n, sw)).all() and (n > 0).all()
        assert R.same_bits(second.hist, first.hist)


def test_rows_with_nothing():
    x = R.score_inputs(4, 300, np.float32, seed=5)
    x["num"][0, :] = 0                                  # no kernels at all
    x["num"][1, :] = 0
    x["num"][1, [3, 200]] = 5
    x["col_valid"][[3, 200]] = 0                        # the only kernels are filtered
    x["num"][2, :] = 0
    cols = [7, 150, 299]
    x["num"][2, cols] = 5
    x["col_valid"][cols] = 1
    x["ref"][x["perm"][7]], x["ref"][x["perm"][150]] = -1.0, np.nan
    x["ref"][x["perm"][299]], x["missing"][x["perm"][299]] = 2.0, 1  # -1, NaN or missing only
    kw = forms(x)["both"]
    want = R.score_terms(x["num"], x["med"], x["avg"], **kw)
    for path in ("partials", "fused"):
        got = run(x, kw, path=path)
        check(got, want)
        assert (got.p[:2] == 0).all() and (got.p[2, :3] == 0).all() and got.p[2, 5] == 3
        assert np.isnan(got.sr[:3]).all() and np.isnan(got.si[:2]).all()
        assert not got.mr[:3].any() and not got.mi[:2].any() and got.err == 0


def test_a_reference_of_zero_is_a_reference():
    # only -1 (any negative) and NaN mean "none": 0.0 counts, with a term of 0
    x = _clean(2, 300, np.float32)
    ref = x["ref"].copy()
    ref[[0, 17, 299]] = 0.0
    kw = dict(ref=ref)
    want = R.score_terms(x["num"], x["med"], x["avg"], **kw)
    assert (want.partials[:, 2] == 300).all()
    for path in ("partials", "fused"):
        check(run(x, kw, path=path), want)
    x["num"][1, 1:] = 0  # a row whose only reference is 0.0: score 0, a straggler
    ref[1:] = -0.0       # -0.0 >= 0 too
    want = R.score_terms(x["num"], x["med"], x["avg"], ref=ref)
    for path in ("partials", "fused"):
        got = run(x, dict(ref=ref), path=path)
        check(got, want)
        assert got.p[1, 2] == 1 and got.sr[1] == 0.0 and got.mr[1] == 1 and got.err == 0


def test_no_columns_is_a_no_op_with_nan_scores():
    # nvrx_scores accepts K == 0 (null arrays allowed): zero partials, NaN scores, no straggler
    x = dict(num=np.zeros((3, 0), np.int32), med=np.zeros((3, 0), np.float32),
             avg=np.zeros((3, 0), np.float32))
    for path in ("partials", "fused"):
        got = run(x, {}, path=path, err0=4)
        assert (got.p == 0).all() and np.isnan(got.sr).all() and np.isnan(got.si).all()
        assert not got.mr.any() and not got.mi.any() and got.err == 4


# ------------------------------------------------------------------ error bits
def _clean(rows, K, dt=np.float64, seed=0):
    """Every kernel present, every column valid, every reference usable."""
    g = np.random.default_rng(seed)
    med = g.uniform(1.0, 100.0, (rows, K)).astype(dt)
    return dict(num=g.integers(1, 40, (rows, K)).astype(np.int32), med=med,
                avg=(med * g.uniform(0.9, 1.4, (rows, K))).astype(dt),
                ref=(med.min(0) * 0.9).astype(np.float32), hist=(med * 1.5).astype(dt))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_zero_med_bit(dt):
    K = 300
    for path in ("partials", "fused"):
        x = _clean(2, K, dt)
        x["med"][1, 40] = 0.0
        assert run(x, dict(ref=x["ref"]), path=path).err == 1       # relative, usable reference
        assert run(x, dict(hist=x["hist"]), path=path).err == 1     # individual: always
        for bad in (-1.0, np.nan):                                  # reference-less column
            ref = x["ref"].copy()
            ref[40] = bad
            assert run(x, dict(ref=ref), path=path).err == 0
            assert run(x, dict(ref=ref, hist=x["hist"]), path=path).err == 1
        miss = np.zeros(K, np.uint32)
        miss[40] = 1
        assert run(x, dict(ref=x["ref"], ref_missing=miss), path=path).err == 0
        valid = np.ones(K, np.uint8)
        valid[40] = 0                                               # filtered column
        assert run(x, dict(ref=x["ref"], hist=x["hist"], col_valid=valid), path=path).err == 0
        for absent in (0, -3):                                      # absent kernel
            x["num"][1, 40] = absent
            assert run(x, dict(ref=x["ref"], hist=x["hist"]), path=path).err == 0
        x["num"][1, 40] = 5
        assert run(x, dict(ref=x["ref"], hist=x["hist"]), path=path, err0=4).err == 4 | 1  # OR-ed


def test_zero_weight_bit():
    x = _clean(3, 257)
    x["avg"][1, :] = 0.0  # n > 0 and sum w == 0; no claim about the score there
    for path in ("partials", "fused"):
        for kw in (dict(ref=x["ref"]), dict(hist=x["hist"]), dict(ref=x["ref"], hist=x["hist"])):
            got = run(x, kw, path=path, err0=4)
            assert got.err == 4 | 2
            assert (got.p[1, [1, 4]] == 0).all()
        x2 = _clean(3, 257)
        x2["avg"][1, :200] = 0.0  # some weight left: no bit
        assert run(x2, dict(ref=x2["ref"], hist=x2["hist"]), path=path, err0=4).err == 4


@pytest.mark.parametrize("rows", [1, 5, 300])
def test_done_epilogue_stores_err_and_resets(rows):
    K, ncols = 600, 37
    for bits, fault in ((0, None), (1, "med"), (2, "avg"), (3, "both")):
        x = _clean(rows, K)
        if fault in ("med", "both"):
            x["med"][rows - 1, 599] = 0.0
        if fault in ("avg", "both"):
            x["avg"][0, :] = 0.0
        done = torch.zeros(2, dtype=torch.int32, device=DEV)
        col_ref = torch.full((2 * ncols,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        kw = dict(ref=x["ref"], hist=x["hist"])
        for _ in range(2):  # the second call starts from what the first left: done == [0, 0]
            got = run(x, kw, path="fused", err0=0x7654, done=done, reset_col_ref=col_ref)
            assert got.err == bits  # stored, not OR-ed
            assert done.cpu().tolist() == [0, 0]
            words = col_ref.cpu().numpy().view(np.uint32)
            assert (words[:ncols] == INF_BITS).all() and (words[ncols:] == 0).all()
            col_ref.fill_(0x5A5A5A5A)
        if fault is None:
            check(got, R.score_terms(x["num"], x["med"], x["avg"], **kw))


# ------------------------------------------------------------------ threshold and rounding order
def test_threshold_is_strict():
    x = dict(num=np.array([[2], [2], [0]], np.int32), med=np.full((3, 1), 4.0),
             avg=np.full((3, 1), 1.5))
    kw = dict(ref=np.array([3.0], np.float32), hist=np.full((3, 1), 3.0))
    up = float(np.nextafter(0.75, 1))
    for path in ("partials", "fused"):
        at = run(x, kw, path=path, thr_rel=0.75, thr_ind=0.75)
        assert at.sr[0] == at.si[1] == 0.75 and np.isnan(at.sr[2]) and np.isnan(at.si[2])
        assert not at.mr.any() and not at.mi.any()            # score == thr: not a straggler
        above = run(x, kw, path=path, thr_rel=up, thr_ind=up)
        assert above.mr.tolist() == [1, 1, 0] and above.mi.tolist() == [1, 1, 0]  # NaN: never
        huge = run(x, kw, path=path, thr_rel=np.inf, thr_ind=np.inf)
        assert huge.mr.tolist() == [1, 1, 0] and huge.mi.tolist() == [1, 1, 0]


def test_mask_follows_the_float32_rounding():
    x = R.rounding_order_row()
    kw = dict(hist=x["hist"])
    for path in ("partials", "fused"):
        plain = run(x, kw, path=path, thr_ind=x["thr"])
        assert plain.si[0] == 0.75 - 2.0 ** -30 and plain.mi[0] == 1
        r32 = run(x, kw, path=path, thr_ind=x["thr"], round_f32=True)
        assert r32.si[0] == 0.75 and r32.mi[0] == 0


# ------------------------------------------------------------------ separately rounded, no FMA
def test_two_term_sums_are_bit_exact():
    """Two present kernels per row, every other term exactly 0: sum t = t0 + t1 and sum w =
    w0 + w1 whatever the reduction order, so they equal numpy's bit for bit -- unless a product
    was fused into the add (test_score_ref_cpu.py shows the inputs tell the two apart)."""
    x = R.two_term_inputs()
    kw = dict(ref=x["ref"], hist=x["hist"])
    want = R.score_terms(x["num"], x["med"], x["avg"], **kw)
    exp = np.zeros((256, 6))
    for r in range(256):
        c0, c1 = x["pairs"][r // 64]
        exp[r] = (want.t_rel[r, c0] + want.t_rel[r, c1], want.w[r, c0] + want.w[r, c1], 2,
                  want.t_ind[r, c0] + want.t_ind[r, c1], want.w[r, c0] + want.w[r, c1], 2)
    for path in ("partials", "fused"):
        got = run(x, kw, path=path)
        bad = np.nonzero((got.p != exp).any(1))[0]
        assert len(bad) == 0, (len(bad), bad[:8], got.p[bad[:2]], exp[bad[:2]])
        with np.errstate(all="ignore"):
            assert R.same_bits(got.sr, exp[:, 0] / exp[:, 1]) and R.same_bits(got.si, exp[:, 3] / exp[:, 4])
        assert R.same_bits(got.hist, want.new_hist)


# ------------------------------------------------------------------ identities
def test_two_runs_are_identical():
    x = R.score_inputs(3, 4097, np.float64, seed=4)
    kw = forms(x)["both"]
    for path in ("partials", "fused"):
        a, b = run(x, kw, path=path), run(x, kw, path=path)  # each from the same initial history
        assert same_result(a, b) and a.err == b.err


def test_three_column_shards_add_up():
    rows, K = 3, 2049
    x = R.score_inputs(rows, K, np.float64, seed=6)
    kw = forms(x)["both"]
    want = R.score_terms(x["num"], x["med"], x["avg"], **kw)
    single = run(x, kw)
    check(single, want)
    shard = np.random.default_rng(6).integers(0, 3, K)
    hist = dev(x["hist"])
    parts = []
    for g in range(3):
        cv = (x["col_valid"] != 0) & (shard == g)
        parts.append(run(x, dict(kw, col_valid=cv.astype(np.uint8)), hist=hist).p)
    stacked = dev(np.stack(parts))
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    gr, gi, mr, mi = ops.finalize_scores(stacked, rows, nshards=3, err=err)
    got = SimpleNamespace(p=np.stack(parts).sum(0), sr=host(gr), si=host(gi), mr=host(mr),
                          mi=host(mi), hist=host(hist))
    assert np.array_equal(got.p[:, [2, 5]], want.partials[:, [2, 5]])
    sr, si, _, _, _ = R.finish(want.partials)
    check_score(got.sr, sr, want.partials[:, 2], 0.75, got.mr, False)
    check_score(got.si, si, want.partials[:, 5], 0.75, got.mi, False)
    assert R.same_bits(got.hist, single.hist) and R.same_bits(got.hist, want.new_hist)
    assert int(err.item()) == 0


# ------------------------------------------------------------------ finalize_scores alone
def _partials(rows, nshards, seed):
    g = np.random.default_rng(seed)
    p = np.zeros((nshards, rows, 6))
    for base in (0, 3):
        n = g.integers(0, 50, (nshards, rows)).astype(np.float64)
        n[g.random((nshards, rows)) < 0.3] = 0
        n[:, 0] = 0                                   # n == 0 in every shard
        w = g.uniform(0.0, 1e4, (nshards, rows)) * (n > 0)
        p[..., base], p[..., base + 1], p[..., base + 2] = w * g.uniform(0.3, 1.0, w.shape), w, n
        last = rows - 1                               # counts in the last shard only
        p[:-1, last, base:base + 3] = 0
        p[-1, last, base:base + 3] = (3.0, 4.0, 2.0)
    return p


@pytest.mark.parametrize("nshards", [1, 2, 3, 5])
@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_finalize_scores_bit_exact(rows, nshards):
    for zero_w in (False, True):
        p = _partials(rows, nshards, seed=rows * 10 + nshards)
        if zero_w:
            r = rows // 2
            p[:, r, 3:5], p[:, r, 5] = 0.0, 1.0       # n > 0, sum w == 0 (individual)
        d = dev(p)
        for round_f32 in (False, True):
            sr, si, mr, mi, zw = R.finalize(p, nshards, round_f32=round_f32, thr_rel=0.6, thr_ind=0.7)
            assert zw == zero_w
            err = torch.full((1,), 4, dtype=torch.int32, device=DEV)
            gr, gi, qr, qi = ops.finalize_scores(d, rows, nshards, round_f32, 0.6, 0.7, err=err)
            assert R.same_bits(host(gr), sr) and R.same_bits(host(gi), si)
            assert np.array_equal(host(qr).astype(bool), mr) and np.array_equal(host(qi).astype(bool), mi)
            assert int(err.item()) == (4 | 2 if zero_w else 4)
            gr, gi, qr, qi = ops.finalize_scores(d, rows, nshards, round_f32, 0.6, 0.7, ind=False)
            assert gi is None and qi is None and R.same_bits(host(gr), sr)
            assert np.array_equal(host(qr).astype(bool), mr)
            gr, gi, qr, qi = ops.finalize_scores(d, rows, nshards, round_f32, 0.6, 0.7, rel=False)
            assert gr is None and qr is None and R.same_bits(host(gi), si)
            assert np.array_equal(host(qi).astype(bool), mi)
    if nshards == 3:  # the order is the shards', starting from 0.0
        q = np.zeros((3, rows, 6))
        q[:, :, 1] = np.array([2.0 ** 53, 1.0, 1.0])[:, None]
        q[0, :, 0], q[:, :, 2] = 2.0 ** 53, 1.0
        for arr in (q, q[::-1]):
            want = R.finalize(arr, 3)[0]
            assert R.same_bits(host(ops.finalize_scores(dev(arr), rows, 3)[0]), want)
        assert R.finalize(q, 3)[0][0] != R.finalize(q[::-1], 3)[0][0]


# ------------------------------------------------------------------ kernel_ref
@pytest.mark.parametrize("K", [1, 255, 256, 257, 600])
@pytest.mark.parametrize("rows", [0, 1, 31, 32, 33, 64, 65, 300])
def test_kernel_ref_bit_exact(rows, K):
    g = np.random.default_rng(rows * 1000 + K)
    num = g.integers(1, 40, (rows, K)).astype(np.int32)
    med = g.uniform(1.0, 100.0, (rows, K)).astype(np.float32)
    if rows:
        med[g.integers(0, rows, K), np.arange(K)] = med.min(0)  # ties of the minimum
        col = lambda i: i % K  # noqa: E731
        for j, r in enumerate(sorted({0, rows // 2, rows - 1})):  # absent in exactly one row:
            num[r, col(3 + j)] = 0 if j % 2 else -2             # first, middle and last chunk
        num[:, col(10)] = 0
        num[rows // 2, col(10)] = 3                             # present in one row only
        med[rows // 3, col(11)] = 0.0                           # MED 0.0 on a present entry
        num[:, col(11)] = 2
        med[:, col(12)] = np.inf                                # +inf on present entries
        num[:, col(12)] = 2
        absent = g.random((rows, K)) < 0.02
        absent[:, [col(11), col(12)]] = False
        num[absent] = g.choice([0, -1], absent.sum())
        poison = np.array([np.nan, np.inf, 0.0, 0.25], np.float32)  # 0.25: below every present MED
        gone = num <= 0
        med[gone] = poison[g.integers(0, 4, gone.sum())]
    want, minbits, missing = R.kernel_ref(num, med)
    assert R.same_bits(want, O.kernel_ref(num, med))
    d_num, d_med = dev(num), dev(med)
    assert R.same_bits(host(ops.kernel_ref(d_num, d_med)), want)
    scratch = torch.full((2 * K,), -1, dtype=torch.int32, device=DEV)
    assert R.same_bits(host(ops.kernel_ref(d_num, d_med, scratch=scratch)), want)
    words = scratch.cpu().numpy().view(np.uint32)
    assert np.array_equal(words[:K], minbits) and np.array_equal(words[K:] != 0, missing != 0)
    if rows >= 31 and K >= 255:
        assert np.isnan(want).any() and (want == 0.0).any() and np.isinf(want).any()


# ------------------------------------------------------------------ stragglers
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_stragglers_equal_numpy(n):
    for thr in (0.75, 0.0, 1.0):
        special = [np.nan, np.inf, -np.inf, 0.0, -0.0, thr, np.nextafter(thr, -np.inf),
                   np.nextafter(thr, np.inf)]
        g = np.random.default_rng(n)
        s = g.uniform(0.0, 1.5, n)
        at = g.permutation(n)[:len(special)]
        s[at] = special[:len(at)] if n > 1 else [thr]
        got = host(ops.stragglers(dev(s), thr))
        assert got.dtype == np.uint8 and np.array_equal(got.astype(bool), R.stragglers(s, thr))
        assert np.array_equal(got, O.stragglers(s, thr))


# ------------------------------------------------------------------ pack_min_times
@pytest.mark.parametrize("total", [1, 255, 256, 257, 262144, 262145, 300001])
def test_pack_min_times_bit_exact(total):
    g = np.random.default_rng(total)
    for n in sorted({0, 1, total // 3, total}):
        ids = g.permutation(total)[:n].astype(np.int32)
        med = g.uniform(0.0, 1e5, n)
        if n:  # halfway between two float32: round to nearest even, both ways
            one = np.float32(1.0)
            med[0] = (float(one) + float(np.nextafter(one, np.float32(2)))) / 2
            med[-1] = med[0] + 2.0 ** -23
        out = torch.full((max(total, 1),), 7.0, dtype=torch.float32, device=DEV)
        got = ops.pack_min_times(dev(med) if n else torch.empty(0, dtype=torch.float64, device=DEV),
                                 dev(ids) if n else torch.empty(0, dtype=torch.int32, device=DEV),
                                 total, out=out)
        assert R.same_bits(host(got), R.pack_min_times(med, ids, total)), n
