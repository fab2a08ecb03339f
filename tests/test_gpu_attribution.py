"""GPU: score attribution (nvrx_score_attribution) from the kernel to the public interfaces.

The checker is numpy in this file: per element, in float64 with separately rounded operations,
    m = MED;  w = NUM * AVG;  s = base / m;  loss = w * (1.0 - s)
over the elements the scores kernel would count (an eligible MED == 0 and a NaN loss are left
out), then a stable descending order (np.argsort(-loss, kind="stable")): idx, loss and score are
compared BIT FOR BIT, wsum within 1e-12 relative (its summation order differs)."""
import math

import numpy as np
import pytest
import torch

from _mp import run_world
from _score_ref import inputs
from nvidia_resiliency_ext.straggler import batch, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------ the numpy checker
def expect(num, med, avg, *, top, kind, col_valid=None, ref=None, ref_index=None, ref_missing=None,
           hist=None, hist_index=None, hist_stride=0):
    R, K = med.shape
    idx = np.full((R, top), -1, np.int32)
    loss = np.full((R, top), np.nan)
    score = np.full((R, top), np.nan)
    wsum = np.zeros(R)
    err = 0
    cols = np.arange(K)
    for r in range(R):
        m = med[r].astype(np.float64)
        w = num[r].astype(np.float64) * avg[r].astype(np.float64)
        elig = num[r] > 0
        if col_valid is not None:
            elig &= col_valid != 0
        if kind == "relative":
            ri = cols if ref_index is None else ref_index
            b32 = ref[ri]
            elig &= b32 >= 0  # -1 and NaN: no reference
            if ref_missing is not None:
                elig &= ref_missing[ri] == 0
            base = b32.astype(np.float64)
        else:
            hi = cols if hist_index is None else hist_index
            base = hist.reshape(-1)[r * (hist_stride or K) + hi].astype(np.float64)
        with np.errstate(all="ignore"):
            s = base / m
            ls = w * (1.0 - s)
        if (elig & (m == 0)).any():
            err |= 1
        take = np.nonzero(elig & (m != 0) & ~np.isnan(ls))[0]
        order = take[np.argsort(-ls[take], kind="stable")][:top]
        n = len(order)
        idx[r, :n], loss[r, :n], score[r, :n] = order, ls[order], s[order]
        wsum[r] = math.fsum(w[take])
    return idx, loss, score, wsum, err


def same_bits(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return (np.array_equal(np.isnan(got), nan) and
            np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(num, med, avg, *, top, kind, **kw):
    """The kernel on host arrays -> host results + the error word + the history afterwards."""
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    d = {k: dev(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    res = ops.score_attribution(dev(num), dev(med), dev(avg), top=top, kind=kind, err=err, **d)
    hist_after = d["hist"].cpu().numpy() if d.get("hist") is not None else None
    return (res.idx.cpu().numpy(), res.loss.cpu().numpy(), res.score.cpu().numpy(),
            res.wsum.cpu().numpy(), int(err.item()), hist_after)


def check(num, med, avg, *, top, kind, **kw):
    gi, gl, gs, gw, gerr, hist_after = run(num, med, avg, top=top, kind=kind, **kw)
    wi, wl, ws, ww, werr = expect(num, med, avg, top=top, kind=kind, **kw)
    tag = (med.shape, str(med.dtype), top, kind)
    assert gi.dtype == np.int32 and gi.shape == wi.shape and np.array_equal(gi, wi), tag
    assert same_bits(gl, wl), tag
    assert same_bits(gs, ws), tag
    np.testing.assert_allclose(gw, ww, rtol=1e-12, atol=0, err_msg=str(tag))
    assert gerr == werr, tag
    if kw.get("hist") is not None:  # read only
        assert np.array_equal(hist_after.view(np.uint8), kw["hist"].view(np.uint8)), tag
    return gi, gl, gs, gw


# ------------------------------------------------------------------ kernel
@pytest.mark.parametrize("K", [1, 7, 255, 256, 257, 2049])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_kernel_matches_numpy(dt, K):
    for R in (1, 3):
        x = inputs(R, K, dt, seed=1000 * R + K)
        n, m, a = x["num"], x["med"], x["avg"]
        for top in (1, 4, 8, 16):
            check(n, m, a, top=top, kind="relative", col_valid=x["col_valid"], ref=x["ref"],
                  ref_index=x["perm"], ref_missing=x["missing"])
            check(n, m, a, top=top, kind="individual", col_valid=x["col_valid"], hist=x["hist"],
                  hist_index=x["slot"], hist_stride=x["stride"])
        # the plain forms: no filter, no index, history rows of K
        check(n, m, a, top=8, kind="relative", ref=x["ref"])
        check(n, m, a, top=8, kind="individual", hist=np.ascontiguousarray(x["hist"][:, :K]))
        # other tops take the next template up
        check(n, m, a, top=3, kind="relative", ref=x["ref"])
        check(n, m, a, top=11, kind="relative", ref=x["ref"])


def test_padding_when_top_exceeds_the_eligible():
    x = inputs(2, 7, np.float32, seed=5)
    x["num"][0, :] = 0            # a row with nothing: all padding, wsum 0
    x["num"][1, :3] = 4
    x["num"][1, 3:] = 0
    gi, gl, gs, gw = check(x["num"], x["med"], x["avg"], top=16, kind="relative",
                           ref=np.full(7, 0.5, np.float32))
    assert (gi[0] == -1).all() and np.isnan(gl[0]).all() and np.isnan(gs[0]).all() and gw[0] == 0.0
    assert (gi[1, :3] >= 0).all() and (gi[1, 3:] == -1).all() and np.isnan(gl[1, 3:]).all()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_equal_losses_keep_column_order(dt):
    R, K = 2, 700  # several columns per thread, every wave
    num = np.full((R, K), 3, np.int32)
    med = np.full((R, K), 2.0, dt)
    avg = np.full((R, K), 5.0, dt)
    ref = np.ones(K, np.float32)
    med[1] = 1.0  # row 1 IS the reference everywhere: every loss is 0
    for top in (1, 4, 8, 16):
        gi, gl, gs, _ = check(num, med, avg, top=top, kind="relative", ref=ref)
        assert np.array_equal(gi, np.tile(np.arange(top, dtype=np.int32), (R, 1)))
        assert (gl[0] == 7.5).all() and (gs[0] == 0.5).all()
        assert (gl[1] == 0.0).all() and (gs[1] == 1.0).all()
    # a larger loss late in the row still comes first, and the ties behind it stay in order
    med[0, 699] = 4.0
    gi, _, _, _ = check(num, med, avg, top=4, kind="relative", ref=ref)
    assert gi[0].tolist() == [699, 0, 1, 2]


def test_negative_and_signed_zero_losses():
    K = 300
    g = np.random.default_rng(9)
    num = np.full((1, K), 2, np.int32)
    med = g.uniform(1.0, 10.0, (1, K)).astype(np.float32)
    avg = med.copy()
    ref = (med[0] * g.uniform(1.05, 1.5, K)).astype(np.float32)  # a caller's reference above MED
    ref[10], ref[200] = med[0, 10], med[0, 200]                  # loss +0.0
    avg[0, 5] = 0.0                                              # loss -0.0 (w = 0, 1 - s < 0)
    ref[5] = 2 * med[0, 5]
    gi, gl, _, _ = check(num, med, avg, top=16, kind="relative", ref=ref)
    assert gi[0, :3].tolist() == [5, 10, 200]  # -0.0 == +0.0: the lower column first
    assert np.signbit(gl[0, 0]) and not np.signbit(gl[0, 1])
    assert (gl[0, 3:] < 0).all() and (np.diff(gl[0]) <= 0).all()


def test_nan_avg_and_zero_med_are_left_out():
    x = inputs(3, 257, np.float64, seed=77)
    x["num"][:, [4, 9, 100]] = 7
    x["avg"][1, 4] = np.nan        # loss NaN: left out like an absent kernel
    x["med"][2, 9] = 0.0           # eligible MED == 0: left out, err |= 1
    x["med"][0, 100] = 0.0
    x["num"][0, 100] = 0           # MED == 0 on an absent kernel: no error from this one
    ref = np.full(257, 0.5, np.float32)
    gi, gl, _, gw = check(x["num"], x["med"], x["avg"], top=16, kind="relative", ref=ref)
    assert np.isfinite(gw).all() and not np.isnan(gl).any()
    *_, err, _ = run(x["num"], x["med"], x["avg"], top=16, kind="relative", ref=ref)
    assert err & 1
    x["med"][2, 9] = 1.0
    *_, err, _ = run(x["num"], x["med"], x["avg"], top=16, kind="relative", ref=ref)
    assert err == 0
    # a NaN AVG or zero MED among few kernels: the column never shows up
    num = np.full((1, 4), 2, np.int32)
    med = np.array([[2.0, 0.0, 2.0, 2.0]])
    avg = np.array([[1.0, 1.0, np.nan, 3.0]])
    gi, _, _, gw = check(num, med, avg, top=4, kind="individual", hist=np.ones((1, 4)))
    assert gi[0].tolist() == [3, 0, -1, -1] and gw[0] == 8.0


def test_two_calls_give_identical_results():
    x = inputs(3, 2049, np.float32, seed=3)
    kw = dict(top=16, kind="relative", col_valid=x["col_valid"], ref=x["ref"], ref_index=x["perm"],
              ref_missing=x["missing"])
    a = run(x["num"], x["med"], x["avg"], **kw)
    b = run(x["num"], x["med"], x["avg"], **kw)
    assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2])
    assert np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64))  # wsum: a fixed order


def test_ops_wrapper_argument_errors():
    t = torch.ones((1, 4), device=DEV)
    n = torch.ones((1, 4), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="ref"):
        ops.score_attribution(n, t, t, top=2, kind="relative")
    with pytest.raises(ValueError, match="hist"):
        ops.score_attribution(n, t, t, top=2, kind="individual")
    with pytest.raises(ValueError, match="device"):
        ops.score_attribution(n.cpu(), t, t, top=2, kind="relative", ref=t[0])


# ------------------------------------------------------------------ decomposition
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("K", [1, 5, 16])
def test_losses_sum_to_one_minus_score(dt, K):
    R = 3
    x = inputs(R, K, dt, seed=40 + K)
    x["num"][:, 0] = 5  # every row scores something: column 0 counts for both kinds
    x["col_valid"][0] = 1
    x["missing"][x["perm"][0]] = 0
    ref = x["ref"].copy()
    ref[x["perm"][0]] = 0.5
    hist = x["hist"].copy()
    hist[0, x["slot"]] = 1e9  # row 0's history is above MED: the scores call lowers it first
    num, med, avg, d_hist = dev(x["num"]), dev(x["med"]), dev(x["avg"]), dev(hist)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    common = dict(col_valid=dev(x["col_valid"]), ref=dev(ref), ref_index=dev(x["perm"]),
                  ref_missing=dev(x["missing"]), hist=d_hist, hist_index=dev(x["slot"]),
                  hist_stride=x["stride"])
    p = ops.scores(num, med, avg, err=err, **common)
    gr, gi, _, _ = ops.finalize_scores(p, R, err=err)
    assert d_hist[0, int(x["slot"][0])] == med[0, 0]
    for kind, want in (("relative", gr), ("individual", gi)):
        kw = {k: v for k, v in common.items()
              if k.startswith("ref") == (kind == "relative") or k == "col_valid"}
        res = ops.score_attribution(num, med, avg, top=16, kind=kind, **kw)
        loss, wsum = res.loss.cpu().numpy(), res.wsum.cpu().numpy()
        got = 1.0 - np.nansum(loss, axis=1) / wsum
        want = want.cpu().numpy()
        scored = ~np.isnan(want)
        assert scored[0] and np.array_equal(wsum > 0, scored)
        np.testing.assert_allclose(got[scored], want[scored], rtol=0, atol=1e-12)
    assert int(err.item()) == 0


# ------------------------------------------------------------------ MatrixReporter
def durations(R, K, S, seed, spread=0.01):
    """[R][K][S] int32 ns: one base duration per kernel, +-1 % per sample."""
    g = np.random.default_rng(seed)
    base = g.uniform(100_000, 200_000, (1, K, 1))
    return base * g.uniform(1 - spread, 1 + spread, (R, K, S))


def check_reporter(rep, att, top, kind):
    """Every array of a BatchAttribution against the numpy recomputation from rep.stats."""
    R, K = rep.R, rep.K
    st = rep.stats.cpu()
    num, med, avg = (getattr(st, f).numpy().reshape(R, K) for f in ("num", "med", "avg"))
    kw = {}
    if kind == "relative":
        present = (num > 0).all(0)
        kw["ref"] = np.where(present, np.where(num > 0, med, np.inf).min(0), np.nan).astype(np.float32)
    else:
        kw["hist"] = rep.hist.cpu().numpy()
    wi, wl, ws, ww, werr = expect(num, med, avg, top=top, kind=kind, **kw)
    assert att.kernel.dtype == np.int32 and np.array_equal(att.kernel, wi)
    assert same_bits(att.loss_us, wl) and same_bits(att.score, ws)
    np.testing.assert_allclose(att.wsum, ww, rtol=1e-12, atol=0)
    assert same_bits(att.share, att.loss_us / att.wsum[:, None])
    assert att.err == werr == 0
    assert att.loss_us.shape == att.score.shape == att.share.shape == (R, top) and att.wsum.shape == (R,)


def test_reporter_names_the_slowed_kernels():
    R, K, S = 4, 40, 32
    d = durations(R, K, S, seed=11)
    d[2, 3] *= 1.5
    d[2, 17] *= 3.0
    ns = dev(d.astype(np.int32))
    rep = batch.MatrixReporter(R, K)
    res = rep.report(ns, S)
    att = rep.attribute(top=2)
    assert att.kernel[2].tolist() == [17, 3]
    check_reporter(rep, att, 2, "relative")
    # the shares of ALL kernels of a rank sum to 1 - score
    full = rep.attribute(top=16)
    check_reporter(rep, full, 16, "relative")
    assert (np.nansum(full.share, axis=1) <= 1 - res.gpu_relative + 1e-12).all()
    # individual, after a second report in which kernel 5 takes twice as long on every rank
    d[:, 5] *= 2.0
    res2 = rep.report(dev(d.astype(np.int32)), S)
    ind = rep.attribute(top=3, kind="individual")
    check_reporter(rep, ind, 3, "individual")
    assert (ind.kernel[:, 0] == 5).all() and np.allclose(ind.score[:, 0], 0.5, rtol=0.03)
    assert (np.nansum(ind.share, axis=1) <= 1 - res2.gpu_individual + 1e-12).all()
    check_reporter(rep, rep.attribute(top=2, kind="relative"), 2, "relative")


def test_reporter_many_ranks_separate_reference():
    R, K, S = 300, 5, 8  # above FUSED_REF_MAX_ROWS: the report's reference is a column reduction
    assert R > batch.FUSED_REF_MAX_ROWS
    d = durations(R, K, S, seed=12, spread=0.2)
    d[123, 4] *= 4.0
    rep = batch.MatrixReporter(R, K)
    rep.report(dev(d.astype(np.int32)), S)
    att = rep.attribute(top=8)  # top > K: padding
    check_reporter(rep, att, 8, "relative")
    assert att.kernel[123, 0] == 4 and (att.kernel[:, 5:] == -1).all()
    check_reporter(rep, rep.attribute(top=1, kind="individual"), 1, "individual")


def test_reporter_record_streams():
    R, K, per = 3, 6, 4
    g = np.random.default_rng(13)
    slot = np.tile(np.repeat(np.arange(K), per), R)
    g.shuffle(slot[:K * per])  # push order within a stream is arbitrary
    ns = g.integers(50_000, 60_000, R * K * per)
    ns[(np.arange(R * K * per) // (K * per) == 1) & (slot == 2)] *= 3  # rank 1 slow on kernel 2
    recs = dev(np.stack([slot, ns], axis=1).astype(np.int32))
    rec_off = torch.arange(R + 1, dtype=torch.int64, device=DEV) * (K * per)
    rep = batch.MatrixReporter(R, K)
    rep.report_records(recs, rec_off)
    att = rep.attribute(top=4)
    check_reporter(rep, att, 4, "relative")
    assert att.kernel[1, 0] == 2


def test_reporter_refuses_what_it_was_not_built_for():
    rep = batch.MatrixReporter(2, 3, relative=False)
    with pytest.raises(RuntimeError, match="relative"):
        rep.attribute(top=2, kind="relative")
    rep = batch.MatrixReporter(2, 3, individual=False)
    with pytest.raises(RuntimeError, match="individual"):
        rep.attribute(top=2, kind="individual")
    with pytest.raises(ValueError, match="top"):
        rep.attribute(top=17)
    with pytest.raises(ValueError, match="kind"):
        rep.attribute(kind="sections")


def test_attribution_disturbs_no_report_buffer():
    R, K, S = 4, 40, 32
    d = durations(R, K, S, seed=14, spread=0.3)
    ns1, ns2 = dev(d.astype(np.int32)), dev((d * 1.1).astype(np.int32))
    plain, probed = batch.MatrixReporter(R, K), batch.MatrixReporter(R, K)
    plain.report(ns1, S)
    probed.report(ns1, S)
    probed.attribute(top=8)
    probed.attribute(top=8, kind="individual")
    a, b = plain.report(ns2, S), probed.report(ns2, S)
    assert same_bits(a.gpu_relative, b.gpu_relative) and same_bits(a.gpu_individual, b.gpu_individual)
    assert np.array_equal(a.stragglers_relative, b.stragglers_relative) and a.err == b.err == 0
    assert torch.equal(plain.hist, probed.hist)


# ------------------------------------------------------------------ ReportGenerator
def test_report_generator_names_the_slowed_kernel():
    from nvidia_resiliency_ext import straggler
    from _report_workers import get_summary

    rg = straggler.reporting.ReportGenerator(['individual_perf_scores'], gather_on_rank0=False,
                                             node_name='testnode')
    with pytest.raises(RuntimeError, match="report"):
        rg.kernel_attribution()
    a, b = np.array([1.0, 1.0, 2.0]), np.array([2.0, 2.0, 3.0])
    rg.generate_report({}, kernel_summaries={'a': get_summary(a), 'b': get_summary(b)})
    first = rg.kernel_attribution(top=8, kind="individual")
    assert [e.name for e in first] == ['a', 'b'] and all(e.loss_us == 0.0 for e in first)  # no padding
    rep = rg.generate_report({}, kernel_summaries={'a': get_summary(a), 'b': get_summary(2 * b)})
    top1 = rg.kernel_attribution(top=1, kind="individual")
    assert len(top1) == 1 and isinstance(top1[0], straggler.KernelAttribution)
    assert top1[0].name == 'b' and top1[0].score == 0.5
    # loss = NUM * AVG * (1 - 0.5); the shares of both kernels sum to 1 - score
    assert top1[0].loss_us == 3 * np.mean(2 * b) * 0.5
    both = rg.kernel_attribution(top=16, kind="individual")
    assert [e.name for e in both] == ['b', 'a'] and both[1].score == 1.0
    assert sum(e.share for e in both) == pytest.approx(1 - rep.gpu_individual_perf_scores[0], abs=1e-12)
    with pytest.raises(RuntimeError, match="relative"):
        rg.kernel_attribution(kind="relative")  # not among scores_to_compute
    with pytest.raises(ValueError, match="top"):
        rg.kernel_attribution(top=0)
    # the history is as the report left it: the next report scores as if nobody had asked
    assert rg.min_local_kernel_times['b'] == 2.0
    rep = rg.generate_report({}, kernel_summaries={'a': get_summary(a), 'b': get_summary(b)})
    assert rep.gpu_individual_perf_scores[0] == pytest.approx(1.0)


def test_report_generator_two_ranks_relative():
    res = run_world(2, "_attribution_workers", "rel_attribution")
    assert res[0]["score"] == pytest.approx(1.0) and res[1]["score"] == pytest.approx(0.5)
    assert [(n, s, l) for n, s, l, _ in res[0]["att"]] == [("kernel0", 1.0, 0.0), ("kernel1", 1.0, 0.0)]
    # rank 1 takes twice as long on both: kernel1 carries the larger weight (3 * 14/3 vs 3 * 8/3)
    (n0, s0, l0, h0), (n1, s1, l1, h1) = res[1]["att"]
    assert (n0, n1) == ("kernel1", "kernel0") and s0 == s1 == 0.5
    assert l0 == pytest.approx(7.0, rel=1e-12) and l1 == pytest.approx(4.0, rel=1e-12)
    assert h0 + h1 == pytest.approx(1 - res[1]["score"], abs=1e-12)


# ------------------------------------------------------------------ Detector
def test_detector_kernel_attribution():
    from _attribution_workers import SLOWED

    first, second = run_world(1, "_attribution_workers", "detector_attribution")[0]
    for r in (first, second):
        for key, score in (("rel", r["rel_score"]), ("ind", r["ind_score"])):
            assert r[key] and all(n in r["names"] for n, *_ in r[key])
            assert sum(h for *_, h in r[key]) <= 1 - score + 1e-12
        assert len(r["rel"]) == len(r["names"]) == 3 and len(r["ind"]) == 2  # top=8 default: no padding
        assert r["again"] == r["ind"]
        assert all(s == 1.0 and l == 0.0 for _, s, l, _ in r["rel"])  # a world of one is its own best
    assert all(l == 0.0 for _, _, l, _ in first["ind"])
    name, score, loss, share = second["ind"][0]
    assert name == SLOWED and score == pytest.approx(0.5, rel=1e-3) and loss > 0
    assert share == pytest.approx(1 - second["ind_score"], abs=1e-12)  # the only kernel that lost
