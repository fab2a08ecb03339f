"""GPU: nvrx_compact_history_from_dense / nvrx_compact_history_to_dense against the host twins
(``histograms.compact_from_dense`` / ``compact_to_dense``) on hand-built elements -- empty, 1, 12,
13 and 240 used buckets, a saturating fold, the bucket rule's ends -- over shapes with a short last
trip and several waves: bytes equal, no tolerance.  Both round-trip identities, ``folded = NULL``,
and a target poisoned with 0xFF that must be overwritten in full, with a guard behind it."""
import numpy as np
import pytest
import torch

from nvidia_resiliency_ext.straggler import histograms, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
BINS, CB = 240, histograms.CHIST_BYTES
U32 = 2 ** 32 - 1

ELEMENTS = (
    {},                                                    # empty: the all-zero element
    {0: 1},
    {239: U32},
    {117: 9},
    {10 * (i + 1): 5 + i for i in range(12)},              # 12: nothing folds
    {3: 1, **{20 * i + 4: 2 for i in range(11)}, 238: 7},  # 13: bucket 238 folds into 204
    {b: b + 1 for b in range(BINS)},                       # 240: 228 buckets fold into bucket 11
    {0: 2, 3: 1, 4: 1, 63: 5, 64: 6, 237: 1, 238: 2, 239: 3},  # lane and row boundaries
    # a saturating fold: the 12th bucket holds 0x10, three bins of 0xFFFFFFF0 above it
    {**{i + 1: 1 for i in range(11)}, 120: 0x10, 130: 0xFFFFFFF0, 140: 0xFFFFFFF0, 150: 0xFFFFFFF0},
    {**{2 * i: U32 for i in range(12)}, 100: U32, 200: U32},  # the fold target is saturated already
)


def dense_history(R, S, shift=0):
    h = np.zeros((R, S, BINS), np.uint32)
    for r in range(R):
        for s in range(S):
            for b, v in ELEMENTS[(3 * r + s + shift) % len(ELEMENTS)].items():
                h[r, s, b] = v
    return h


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(DEV)


def poisoned(shape, dtype):
    """A target filled with 0xFF with a 64-byte guard behind it: (the view, the whole)."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    whole = torch.full((n + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    return whole[:n].view(dtype).view(shape), whole


SHAPES = ((1, 1), (1, 13), (3, 37), (2, 50), (70, 3))


@pytest.mark.parametrize("R,S", SHAPES)
def test_from_dense_equals_the_twin_and_overwrites_its_target(R, S):
    h = dense_history(R, S)
    want, wf = histograms.compact_from_dense(h)
    assert wf.any() or R * S < 6
    out, whole = poisoned((R, S, CB), torch.uint8)
    folded = torch.full((R,), -7, dtype=torch.int64, device=DEV)
    got, f = ops.compact_history_from_dense(dev(h, np.int32), out=out, folded=folded)
    assert got is out and f is folded
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(folded.cpu().numpy().view(np.uint64), wf)
    assert whole[-64:].cpu().tolist() == [0xFF] * 64
    assert histograms.compact_is_canonical(out.cpu().numpy()).all()
    # folded = NULL is accepted, and the elements are the same
    out2, whole2 = poisoned((R, S, CB), torch.uint8)
    got2, f2 = ops.compact_history_from_dense(dev(h, np.int32), out=out2, folded=False)
    assert f2 is None and torch.equal(out2, out) and whole2[-64:].cpu().tolist() == [0xFF] * 64


@pytest.mark.parametrize("R,S", SHAPES)
def test_to_dense_equals_the_twin_and_overwrites_its_target(R, S):
    ch, _ = histograms.compact_from_dense(dense_history(R, S, shift=1))
    want = histograms.compact_to_dense(ch)
    out, whole = poisoned((R, S, BINS), torch.int32)
    got = ops.compact_history_to_dense(dev(ch, np.uint8), out=out)
    assert got is out
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
    assert whole[-64:].cpu().tolist() == [0xFF] * 64


def test_round_trips():
    # to_dense(from_dense(H)) == H exactly when no element of H uses more than 12 buckets
    rows = [e for e in ELEMENTS if len(e) <= 12]
    h = np.zeros((2, len(rows), BINS), np.uint32)
    for s, e in enumerate(rows):
        for b, v in e.items():
            h[0, s, b] = v
            h[1, len(rows) - 1 - s, b] = v
    d_h = dev(h, np.int32)
    ch, folded = ops.compact_history_from_dense(d_h)
    assert folded.cpu().tolist() == [0, 0]
    assert torch.equal(ops.compact_history_to_dense(ch), d_h)
    # from_dense(to_dense(c)) == c for every canonical c, folded ones included
    c0, f0 = ops.compact_history_from_dense(dev(dense_history(3, 37), np.int32))
    assert f0.cpu().numpy().any()
    c1, f1 = ops.compact_history_from_dense(ops.compact_history_to_dense(c0))
    assert torch.equal(c1, c0) and f1.cpu().tolist() == [0, 0, 0]


def test_wrappers_reject_wrong_shapes_and_types():
    h = torch.zeros((2, 3, BINS), dtype=torch.int32, device=DEV)
    c = torch.zeros((2, 3, CB), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="hist"):
        ops.compact_history_from_dense(c)
    with pytest.raises(ValueError, match="chist"):
        ops.compact_history_to_dense(h)
    with pytest.raises(ValueError, match="out"):
        ops.compact_history_from_dense(h, out=c[:1])
    with pytest.raises(ValueError, match="out"):
        ops.compact_history_to_dense(c, out=h[:, :2])
    with pytest.raises(ValueError, match="folded"):
        ops.compact_history_from_dense(h, folded=torch.zeros(3, dtype=torch.int64, device=DEV))
