"""GPU: the chain a ``half_life`` call runs -- age, then score and update -- on the device against
the same chain on the host, interval by interval, for a few never-folding and a few folding cases
of ``_compact_history_cases``:

    device  nvrx_compact_history_age -> nvrx_segment_history_scores_compact_ragged (SCORE | UPDATE)
    host    histograms.compact_age   -> histograms.segment_compact_history_scores

Integers equal, f64 bit patterns equal, the whole history equal; no tolerance.  For the
never-folding cases the dense device chain (nvrx_histogram_history_age ->
nvrx_segment_history_scores_ragged) gives the same bits and the same history, expanded: the
bit-identity of the two histories survives aging.  The slots no column uses start empty here
(aging concerns every slot, and the cases' sentinel pattern is not a canonical element)."""
import functools

import numpy as np
import pytest
import torch

import _compact_history_cases as C
from nvidia_resiliency_ext.straggler import histograms, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -7
SUMS = ("tail_ns", "total_ns", "base_tail_ns", "base_total_ns")
NEVER_FOLD = ("cap_trims", "hist_index_permuted", "stride_above_K", "skip_rows", "saturation",
              "col_valid_K17")
FOLD = ("fold_rule", "lengths_unaligned", "compact_cap_trims", "skip_and_invalid", "special_keys")
RUNS = [(n, s) for n in NEVER_FOLD + FOLD for s in (1, 2)]


def dev(a, dt=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(DEV)


def start(c):
    """The case's starting history with the slots no column uses empty."""
    S = c.stride or c.K
    h = c.chist0.copy()
    h[:, sorted(set(range(S)) - set(C.used_slots(c)))] = 0
    return h


@functools.lru_cache(maxsize=None)
def host_chain(name, shift):
    """Per interval: (the aged history, evicted, full, the twin's fused result on it)."""
    c = C.case(name)
    h, out = start(c), []
    for iv in c.intervals:
        aged, ev, fu = histograms.compact_age(h, shift)
        res = histograms.segment_compact_history_scores(iv.keys, iv.off, iv.lens, c.K, aged, c.pm,
                                                        cap=iv.cap, score_thr=C.THR,
                                                        **C.history_kwargs(c))
        out.append((aged, ev, fu, res))
        h = res.hist
    return tuple(out)


def sentinel_out(R):
    i = lambda: torch.full((R,), SENT, dtype=torch.int64, device=DEV)  # noqa: E731
    return ops.HistoryTailScores(torch.full((R,), float(SENT), dtype=torch.float64, device=DEV),
                                 i(), i(), i(), i(), torch.full((R,), 9, dtype=torch.uint8, device=DEV))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_the_chosen_cases_fold_and_do_not_fold_under_aging():
    for name, shift in RUNS:
        folds = sum(int(res.folded.sum()) for _, _, _, res in host_chain(name, shift))
        assert (folds == 0) == (name in NEVER_FOLD), (name, shift, folds)


@pytest.mark.parametrize("name,shift", RUNS)
def test_age_then_score_and_update_equals_the_host_chain(name, shift):
    c = C.case(name)
    opt = lambda v, dt: None if v is None else torch.as_tensor(np.asarray(v), dtype=dt).to(DEV)  # noqa: E731
    d_chist = dev(start(c), np.uint8)
    d_hist = dev(histograms.compact_to_dense(start(c))) if name in NEVER_FOLD else None
    for iv, (aged, ev, fu, twin) in zip(c.intervals, host_chain(name, shift)):
        keys, off, lens = dev(iv.keys), dev(iv.off, np.int64), dev(iv.lens)
        kw = dict(hist_index=opt(c.hist_index, torch.int32), hist_stride=c.stride,
                  col_valid=opt(c.col_valid, torch.uint8), skip_rows=opt(c.skip_rows, torch.uint8),
                  permille=c.pm, cap=iv.cap, aligned16=iv.aligned16, score_thr=C.THR)
        evicted, full = ops.compact_history_age(d_chist, shift)
        assert np.array_equal(d_chist.cpu().numpy(), aged)
        assert np.array_equal(evicted.cpu().numpy().view(np.uint64), ev)
        assert np.array_equal(full.cpu().numpy().view(np.uint64), fu)
        res, folded = ops.segment_history_scores_compact_ragged(
            keys, off, lens, c.K, max(iv.max_len, 1), d_chist, tail_calls=True,
            out=sentinel_out(c.R), **kw)
        for n in SUMS:
            assert np.array_equal(getattr(res, n).cpu().numpy().view(np.uint64), getattr(twin, n)), n
        assert res.score.cpu().numpy().tobytes() == twin.score.tobytes()
        assert res.strag.cpu().numpy().astype(bool).tolist() == twin.stragglers.tolist()
        assert np.array_equal(res.tail_calls.cpu().numpy().view(np.uint32), twin.tail_calls)
        assert np.array_equal(folded.cpu().numpy().view(np.uint64), twin.folded)
        assert np.array_equal(d_chist.cpu().numpy(), twin.hist)
        if d_hist is not None:  # the dense chain: the same bits, the same history expanded
            ops.histogram_history_age(d_hist, shift)
            want = ops.segment_history_scores_ragged(keys, off, lens, c.K, max(iv.max_len, 1), d_hist,
                                                     tail_calls=True, out=sentinel_out(c.R), **kw)
            for n in SUMS + ("score", "strag", "tail_calls"):
                assert same_bits(getattr(res, n), getattr(want, n)), n
            assert np.array_equal(histograms.compact_to_dense(d_chist.cpu().numpy()),
                                  d_hist.cpu().numpy().view(np.uint32))
