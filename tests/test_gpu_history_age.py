"""GPU: nvrx_compact_history_age and nvrx_histogram_history_age against their host twins
(``histograms.compact_age`` / ``history_age``), byte for byte with a guard region behind the
tensor and no tolerance, at the smallest shapes at which history_age.hip can go wrong: idle DPP
rows (1 x 1), the four-per-wave boundary (1 x 3, 4, 5), one past a 16-element granule (1 x 17), a
wave straddling rows (3 x 5) and several waves (2 x 64); every shape populated from the shared
elements of ``_history_age_cases`` so that each meets every directed element."""
import numpy as np
import pytest
import torch

import _history_age_cases as A
from nvidia_resiliency_ext.straggler import histograms, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 0x5E
SENT = -7
SHAPES = ((1, 1), (1, 3), (1, 4), (1, 5), (1, 17), (3, 5), (2, 64))


def guarded(a):
    """A device copy of a host array with 64 guard bytes behind it: (the view, the whole)."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    whole = torch.full((raw.size + 64,), GUARD, dtype=torch.uint8, device=DEV)
    whole[:raw.size].copy_(torch.from_numpy(raw.copy()).to(DEV))
    view = whole[:raw.size]
    if a.dtype != np.uint8:
        view = view.view(torch.int32)
    return view.view(a.shape), whole


def guard_ok(whole):
    return whole[-64:].cpu().tolist() == [GUARD] * 64


def sentinels(R):
    return (torch.full((R,), SENT, dtype=torch.int64, device=DEV),
            torch.full((R,), SENT - 1, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("R,S", SHAPES)
def test_compact_equals_the_twin(R, S):
    for phase in A.phases(R, S):
        h = A.history(R, S, phase)
        for shift in A.SHIFTS:
            want, ev, fu = A.aged(R, S, phase, shift)
            # sentinel-filled outputs: cleared, not accumulated
            d, whole = guarded(h)
            evicted, full = sentinels(R)
            got = ops.compact_history_age(d, shift, evicted=evicted, full=full)
            assert got[0] is evicted and got[1] is full
            assert guard_ok(whole)
            assert np.array_equal(d.cpu().numpy(), want), (phase, shift)
            assert np.array_equal(evicted.cpu().numpy().view(np.uint64), ev), (phase, shift)
            assert np.array_equal(full.cpu().numpy().view(np.uint64), fu), (phase, shift)
            # NULL outputs
            d, whole = guarded(h)
            assert ops.compact_history_age(d, shift, counts=False) == (None, None)
            assert guard_ok(whole)
            assert np.array_equal(d.cpu().numpy(), want), (phase, shift)


def test_compact_outputs_allocated_by_the_wrapper():
    R, S = 3, 5
    d, _ = guarded(A.history(R, S))
    evicted, full = ops.compact_history_age(d)  # shift 1
    _, ev, fu = A.aged(R, S, 0, 1)
    assert evicted.dtype == full.dtype == torch.int64
    assert np.array_equal(evicted.cpu().numpy().view(np.uint64), ev)
    assert np.array_equal(full.cpu().numpy().view(np.uint64), fu)


@pytest.mark.parametrize("R,S", [(1, 1), (1, 5), (3, 5), (2, 64)])
def test_an_empty_history_is_not_written(R, S):
    """Elements with n = 0 are not stored: a guard pattern inside their own count and bucket bytes
    survives, and an all-zero history stays all zero with the guard behind it intact."""
    h = np.full((R, S, A.CB), GUARD, np.uint8)
    h[..., 5 * A.E:] = 0  # n = 0; the 60 bytes before it hold the guard pattern
    d, whole = guarded(h)
    evicted, full = ops.compact_history_age(d, 1, *sentinels(R))
    assert guard_ok(whole) and np.array_equal(d.cpu().numpy(), h)
    assert evicted.cpu().tolist() == [0] * R and full.cpu().tolist() == [0] * R
    z, whole = guarded(np.zeros((R, S, A.CB), np.uint8))
    ops.compact_history_age(z, 31, counts=False)
    assert guard_ok(whole) and not z.any().item()


def test_empty_elements_between_used_ones_are_not_written():
    # rows of one wave trip: used, n = 0 with guard bytes, used, n = 0 with guard bytes, used
    h = A.history(1, 5, 3).copy()  # full elements
    for s in (1, 3):
        h[0, s] = GUARD
        h[0, s, 5 * A.E:] = 0
    want = h.copy()
    aged, _, _ = histograms.compact_age(np.ascontiguousarray(h[:, [0, 2, 4]]), 1)
    want[0, [0, 2, 4]] = aged[0]
    d, whole = guarded(h)
    ops.compact_history_age(d, 1, counts=False)
    assert guard_ok(whole) and np.array_equal(d.cpu().numpy(), want)


def dense_case(R, S):
    rng = np.random.default_rng(31 * R + S)
    d = np.zeros((R, S, A.BINS), np.uint32)
    fill = rng.random(d.shape) < 0.1
    d[fill] = rng.integers(1, 1 << 32, int(fill.sum()), dtype=np.uint64).astype(np.uint32)
    d[0, 0, 0], d[0, 0, 239] = 2 ** 32 - 1, 2 ** 32 - 1
    d[-1, -1, 0], d[-1, -1, 239], d[-1, -1, 1] = 1, 2 ** 32 - 1, 2
    return d


@pytest.mark.parametrize("R,S", [(1, 1), (2, 5)])
@pytest.mark.parametrize("shift", A.SHIFTS)
def test_dense_equals_the_twin(R, S, shift):
    h = dense_case(R, S)
    d, whole = guarded(h.view(np.int32))
    assert ops.histogram_history_age(d, shift) is d
    assert guard_ok(whole)
    assert np.array_equal(d.cpu().numpy().view(np.uint32), histograms.history_age(h, shift))


def test_dense_zero_history_stays_zero():
    d, whole = guarded(np.zeros((2, 5, A.BINS), np.int32))
    ops.histogram_history_age(d, 1)
    assert guard_ok(whole) and not d.any().item()


@pytest.mark.parametrize("shift", A.SHIFTS)
def test_aged_compact_expands_to_the_aged_dense_on_the_device(shift):
    R, S = 2, 64
    h = A.history(R, S)
    c, _ = guarded(h)
    d, _ = guarded(histograms.compact_to_dense(h).view(np.int32))
    ops.compact_history_age(c, shift, counts=False)
    ops.histogram_history_age(d, shift)
    assert np.array_equal(histograms.compact_to_dense(c.cpu().numpy()),
                          d.cpu().numpy().view(np.uint32))


def test_two_identical_calls_give_identical_bits_and_capture_replays():
    R, S = 3, 5
    h = A.history(R, S)
    want, ev, fu = A.aged(R, S, 0, 1)
    d = torch.from_numpy(h.copy()).to(DEV)
    evicted, full = sentinels(R)
    ops.compact_history_age(d, 1, evicted=evicted, full=full)  # the kernels are loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.compact_history_age(d, 1, evicted=evicted, full=full)
    for _ in range(2):
        d.copy_(torch.from_numpy(h.copy()).to(DEV))  # the history is restored between replays
        evicted.fill_(SENT)
        full.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy(), want)
        assert np.array_equal(evicted.cpu().numpy().view(np.uint64), ev)
        assert np.array_equal(full.cpu().numpy().view(np.uint64), fu)


def test_wrappers_reject_a_history_of_the_wrong_shape_or_type():
    for bad in (torch.zeros((1, 2, 60), dtype=torch.uint8, device=DEV),
                torch.zeros((1, 2, 16), dtype=torch.int32, device=DEV)):
        with pytest.raises(ValueError, match="chist"):
            ops.compact_history_age(bad)
    with pytest.raises(ValueError, match="hist"):
        ops.histogram_history_age(torch.zeros((1, 2, 239), dtype=torch.int32, device=DEV))
    ok = torch.zeros((1, 2, 64), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="evicted"):
        ops.compact_history_age(ok, evicted=torch.zeros(2, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="counts=False"):
        ops.compact_history_age(ok, counts=False, full=torch.zeros(1, dtype=torch.int64, device=DEV))
