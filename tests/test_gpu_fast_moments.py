"""GPU parity: FAST-mode AVG / STD against the exact rational moments (tests/_moments_ref.py), at
the bound derived from the kernel's arithmetic, on every FAST path.

AVG must be the correctly rounded float32 of the exact mean (the other neighbour only within the
quotient's 2^-52 of a rounding midpoint).  STD must lie within
`_moments_ref.std_bound` -- about 2.4e-7 (1 + z^2) + 1.5e-7 with z = (pivot - mean) / sigma and the
pivot the median of the first, middle and last retained sample -- and be +0.0 for a constant
segment.  No case accepts the EXACT kernel's values unless the dispatch rule, applied to the
input, sends the segment there (`_moments_cases.sent_to_exact`); then it demands them.

tests/test_moments_ref_cpu.py proves, from the keys alone, the branch each case takes and where
its pivot lies.  Every test prints its worst relative STD error next to the bound.
"""
import numpy as np
import pytest
import torch

import _moments_cases as C
import _moments_ref as M
import oracle as O
from _fastbars import check_avg_std
from nvidia_resiliency_ext.straggler import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(host):
    t = torch.from_numpy(np.ascontiguousarray(host).view(np.int32)).to(DEV)
    assert t.data_ptr() % 16 == 0
    return t


def _verify(tag, items, exact=False, pivot_of=None):
    """items: (name, retained keys, num, min, max, med, avg, std) per segment.  NUM / MIN / MAX /
    MED bit-exact with computeStats; AVG / STD by `_moments_ref.check`, or (exact: the dispatch
    rule sends the segment to the EXACT kernel) computeStats' own bits.  pivot_of: the pivot to
    bound with, where it is not the rule's."""
    failures, worst = [], (0.0, 0.0, "")
    for name, keys, num, mn, mx, med, avg, std in items:
        r = O.compute_stats(O.key_to_us(keys))
        got = [np.float32(v) for v in (mn, mx, med)]
        want = [np.float32(v) for v in (r.min, r.max, r.median)]
        if int(num) != len(keys) or got != want:
            failures.append((name, "num/min/max/med", int(num), got, want))
        if exact:
            if (np.float32(avg), np.float32(std)) != (np.float32(r.avg), np.float32(r.stddev)):
                failures.append((name, "EXACT kernel bits", float(avg), float(std), r.avg, r.stddev))
            continue
        m = M.moments(keys, None if pivot_of is None else pivot_of(keys))
        if not M.avg_ok(avg, m):
            failures.append((name, "avg", float(avg), float(m.avg_f32), m.mid_dist))
        err = M.std_err(std, m)
        bound = M.std_bound(m) if m.sigma2 else 0.0
        if err > bound:
            failures.append((name, "std", float(std), m.std, f"err {err:.3e} bound {bound:.3e} z2 {m.z2:.3g}"))
        if m.sigma2 and err / bound >= worst[0]:
            worst = (err / bound, err, name)
    print(f"[fast-moments] {tag}: {len(items)} segments, worst STD err / bound {worst[0]:.3f} "
          f"(rel err {worst[1]:.3e}, {worst[2]}); failures {len(failures)}")
    for f in failures:
        print(f"[fast-moments]   FAIL {tag}: {f}")
    assert not failures, (tag, failures[:4])


def _items(names, segs, g, idx):
    return [(nm, k, g.num[i].item(), g.min[i].item(), g.max[i].item(), g.med[i].item(),
             g.avg[i].item(), g.std[i].item()) for nm, k, i in zip(names, segs, idx)]


def _strided(segs, n, begin, cap=0, mode=ops.STATS_FAST, length=None):
    """Equal-length segments through segment_stats_strided; the stride is a multiple of 4 slots,
    so the retained runs start on a 16-byte boundary exactly when begin + (length - keep) does."""
    length = length or n
    stride = (begin + length + 3) // 4 * 4
    host = np.full(len(segs) * stride, 8_000_000, np.uint32)
    for i, k in enumerate(segs):
        host[i * stride + begin:i * stride + begin + length] = k
    st = ops.segment_stats_strided(_dev(host), len(segs), stride, begin, length, cap=cap, mode=mode)
    return st.cpu()


# ---------------------------------------------------------------- pivot-outlier family
@pytest.mark.parametrize("begin", [0, 1, 3])
@pytest.mark.parametrize("n", [255, 256, 1000, 1024, 8191, 8192])
def test_family_strided(n, begin):
    """One wave per segment: the unmasked body (begin 0 and n = 64 PL: the group kernel with one
    segment per wave) and the masked one (every other case).  A misaligned run of more than
    8189 samples does not fit a wave and runs the EXACT kernel."""
    fam = C.outlier_family(n)
    g = _strided(list(fam.values()), n, begin)
    exact = C.sent_to_exact(n, begin % 4 == 0)
    assert exact == (n + (3 if begin else 0) > 8192)
    _verify(f"strided n={n} begin={begin}" + (" (EXACT kernel)" if exact else ""),
            _items(fam.keys(), fam.values(), g, range(len(fam))), exact=exact)


def test_family_group_kernel():
    """seg_stats_lean_group_kernel with groups of 4 (test_grouped_full_segments' smallest shape):
    family members at the first, last and middle positions of a group and in the partial last
    group; the random bulk is checked vectorised."""
    n, mult, K = 256, 3601, 37
    nseg = K * mult
    group = min(8, max(1, nseg // 32768))
    assert group == 4 and nseg % group
    rng = np.random.default_rng(n)
    host = rng.integers(2000, 2_200_000, size=nseg * n, dtype=np.uint32)
    fam = C.outlier_family(n)
    where = [0, group - 1, group, 5 * group + 1, 5 * group + 2, nseg - 1, 3 * group - 1, 7 * group + 1,
             nseg // 2 // group * group]
    assert len(where) == len(fam) and len(set(where)) == len(where)
    for w, k in zip(where, fam.values()):
        host[w * n:(w + 1) * n] = k
    g = ops.segment_stats_strided(_dev(host), nseg, n, 0, n, cap=0, mode=ops.STATS_FAST).cpu()
    _verify("group kernel n=256 group=4", _items(fam.keys(), fam.values(), g, where))
    err, bound = M.check_batch(g.avg.numpy(), g.std.numpy(), host.reshape(nseg, n), tag="group bulk")
    print(f"[fast-moments] group bulk: {nseg} segments, worst err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")


@pytest.mark.parametrize("L,W", [(200, 8), (400, 7)])
def test_family_list_classes(L, W):
    """The ragged wave classes of PL 4 / 8 (seg_stats_list_kernel: prefetched loads, a chunk's
    results one per lane) at test_list_chunk_epilogue's counts: chunks of two entries."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    G = 4 * cus * W
    cnt = 2 * 4 * G + 5
    rng = np.random.default_rng(L)
    host = rng.integers(2000, 2_200_000, size=cnt * L, dtype=np.uint32)
    fam = C.outlier_family(L)
    names = list(fam.keys()) * 4
    where = rng.choice(cnt, len(names), replace=False)
    for nm, w in zip(names, where):
        host[w * L:(w + 1) * L] = fam[nm]
    off = np.arange(cnt + 1, dtype=np.int64) * L
    g = ops.segment_stats_ragged(_dev(host), torch.from_numpy(off).to(DEV), None, max_len=L, cap=0,
                                 mode=ops.STATS_FAST, aligned16=True).cpu()
    _verify(f"list class L={L}", _items(names, [fam[nm] for nm in names], g, where))
    err, bound = M.check_batch(g.avg.numpy(), g.std.numpy(), host.reshape(cnt, L), tag=f"list bulk L={L}")
    print(f"[fast-moments] list bulk L={L}: {cnt} segments, worst err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")


@pytest.mark.parametrize("aligned16", [True, False])
def test_family_list_classes_long(aligned16):
    """The ragged wave classes of PL 16 (prefetched) and PL 32 / 128 (plain loads, emit_stats per
    segment), aligned and at every 4-byte phase."""
    rng = np.random.default_rng(5 + aligned16)
    names, segs = [], []
    for L in (1000, 1100, 8189):
        for nm, k in C.outlier_family(L).items():
            names.append(f"{nm} L={L}")
            segs.append(k)
    off, pos = [], 0
    for i, k in enumerate(segs):
        pos += (-pos) % 4 if aligned16 else (i % 4 - pos) % 4
        off.append(pos)
        pos += k.size
    host = rng.integers(2000, 2_200_000, size=pos + 8, dtype=np.uint32)
    for o, k in zip(off, segs):
        host[o:o + k.size] = k
    lens = np.array([k.size for k in segs], np.int32)
    g = ops.segment_stats_ragged(_dev(host), torch.from_numpy(np.array(off, np.int64)).to(DEV),
                                 torch.from_numpy(lens).to(DEV), max_len=int(lens.max()), cap=0,
                                 mode=ops.STATS_FAST, aligned16=aligned16).cpu()
    assert not any(C.sent_to_exact(int(L), aligned16) for L in lens)
    _verify(f"list classes PL 16/32/128 aligned16={aligned16}", _items(names, segs, g, range(len(segs))))


@pytest.mark.parametrize("keep,nfull", [(1024, 4 * 8300 + 3), (8192, 4 * 30 + 3)])
def test_family_full_classes(keep, nfull):
    """The FULL classes (seg_stats_list_full_kernel: rings at or past a capacity of 64 PL samples,
    four list entries per wave): family members at the first, last and middle entry of a group
    and in the partial last group, overflowed rings among them."""
    rng = np.random.default_rng(keep + nfull)
    lens = np.where(rng.random(nfull) < 0.5, keep, keep + 4 * rng.integers(1, 64, nfull)).astype(np.int64)
    off = np.zeros(nfull, np.int64)
    off[1:] = np.cumsum(lens)[:-1]  # lengths are multiples of 4: every retained run 16-B aligned
    host = rng.integers(2000, 2_200_000, size=int(lens.sum()) + 8, dtype=np.uint32)
    fam = C.outlier_family(keep)
    at = [0, 3, 4, 5, nfull // 2, nfull - 1, nfull - 2, nfull - 3, 9]
    assert len(at) == len(fam)
    for a, k in zip(at, fam.values()):
        end = off[a] + lens[a]
        host[off[a]:end] = 8_000_000          # what an overflowed ring dropped is not a probe
        host[end - keep:end] = k
    g = ops.segment_stats_ragged(_dev(host), torch.from_numpy(off).to(DEV),
                                 torch.from_numpy(lens.astype(np.int32)).to(DEV), max_len=int(lens.max()),
                                 cap=keep, mode=ops.STATS_FAST, aligned16=True).cpu()
    _verify(f"FULL class keep={keep}", _items(fam.keys(), fam.values(), g, at))
    idx = (off + lens - keep)[:, None] + np.arange(keep)[None, :]
    err, bound = M.check_batch(g.avg.numpy(), g.std.numpy(), host[idx], tag=f"FULL bulk keep={keep}")
    print(f"[fast-moments] FULL bulk keep={keep}: {nfull} segments, worst err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")


@pytest.mark.parametrize("pushed,cap", [(1500, 1024), (1501, 1024), (9000, 8192), (300, 255)])
def test_family_ring_past_capacity(pushed, cap):
    """A ring that wrapped (cap < pushed): the probes are the first, middle and last *retained*
    sample.  The dropped head holds 8 ms calls, which as probes would break the bound.  1501
    pushes leave the retained run off the 16-byte boundary (masked body)."""
    fam = C.outlier_family(cap)
    segs = [np.concatenate([np.full(pushed - cap, 8_000_000, np.uint32), k]) for k in fam.values()]
    g = _strided(segs, cap, 0, cap=cap, length=pushed)
    aligned = (pushed - cap) % 4 == 0
    assert not C.sent_to_exact(cap, aligned)
    _verify(f"ring pushed={pushed} cap={cap}", _items(fam.keys(), fam.values(), g, range(len(fam))))


def _farthest_median_of_three(keys):
    """Bucketing does not keep a slot's records in push order, so which three samples the probes
    are is not known.  A median of three distinct samples lies between the second smallest and
    the second largest one: the bound takes whichever of the two is farther from the mean."""
    s = np.sort(np.asarray(keys, np.uint32))
    mean = s.astype(np.float64).mean()
    return int(s[1]) if abs(int(s[1]) - mean) >= abs(int(s[-2]) - mean) else int(s[-2])


def test_family_record_stream():
    """ops.records_stats: slots of 300 records whose first record is the outlier (and the rest of
    the family), a slot of 100 records (lane class: computeStats' bits) and one of 1 record."""
    fam = C.outlier_family(300)
    slots = list(fam.values()) + [C.outlier_family(100)["hi@first"], np.array([777], np.uint32)]
    nslots = len(slots)
    order = np.concatenate([np.full(k.size, s, np.int64) for s, k in enumerate(slots)])
    order = order[np.random.default_rng(3).permutation(order.size)]  # pushes interleaved over slots
    nxt = [0] * nslots
    recs = np.empty((order.size, 2), np.uint32)
    for i, s in enumerate(order):
        recs[i] = (s, slots[s][nxt[s]])   # each slot's records in its own push order
        nxt[s] += 1
    off = np.array([0, order.size], np.int64)
    st = ops.records_stats(_dev(recs.reshape(-1)).view(-1, 2), torch.from_numpy(off).to(DEV), nslots, 0,
                           int(order.size), mode=ops.STATS_FAST).cpu()
    ref = O.records_stats(recs, off, nslots, cap=0)
    for f in ("num", "min", "max", "med"):
        assert np.array_equal(getattr(st, f).numpy().view(np.int32), ref[f].view(np.int32)), f
    ms = [M.moments(k, _farthest_median_of_three(k) if k.size > 2 else None) for k in slots]
    xm = np.array([float(m.avg) for m in ms])
    xs = np.array([m.std for m in ms])
    bound = np.array([M.std_bound(m) if m.sigma2 else 0.0 for m in ms])
    check_avg_std(st.avg.numpy(), st.std.numpy(), ref, xm, xs, "family record stream", std_rtol=bound)
    names = list(fam.keys()) + ["hi@first n=100", "single"]
    big = [i for i, k in enumerate(slots) if k.size > 128]
    _verify("record stream, 300 records per slot", _items([names[i] for i in big], [slots[i] for i in big], st, big),
            pivot_of=_farthest_median_of_three)
    for f in ("avg", "std"):  # lane classes: the reference's own bits
        assert np.array_equal(getattr(st, f).numpy()[nslots - 2:].view(np.uint32), ref[f][nslots - 2:].view(np.uint32)), f
    assert st.std.numpy().view(np.uint32)[nslots - 1] == 0


# ---------------------------------------------------------------- one segment per sum branch
@pytest.mark.parametrize("n", [64, 1000, 8192])
def test_branches_and_edge_segments(n):
    """range < 2^23 / < 2^24 / < 2^31 / >= 2^31 below KEY_WIDE / wide keys, and every
    _edge_segments member, each against the bound of its own branch: PL 4 masked (n = 64), PL 16
    masked (1000), PL 128 unmasked (8192)."""
    br = C.branch_family(n)
    edges = C.edge_segments(n)
    names = list(br.keys()) + [f"edge{i}" for i in range(len(edges))]
    segs = list(br.values()) + edges
    g = _strided(segs, n, 0)
    _verify(f"branches n={n}", _items(names, segs, g, range(len(segs))))
    if n == 1000:  # the masked body at another 4-byte phase
        g = _strided(segs, n, 2)
        _verify(f"branches n={n} begin=2", _items(names, segs, g, range(len(segs))))


# ---------------------------------------------------------------- AVG at a rounding midpoint
@pytest.mark.parametrize("n", [1000, 1024])
def test_avg_next_to_a_midpoint(n):
    """The exact mean lies 4e-14 (relative) from an f32 midpoint, on the odd neighbour's side:
    masked body + emit_stats (n = 1000), unmasked body + the lane-parallel epilogue (1024)."""
    k = C.midpoint_segment(n)
    m = M.moments(k)
    g = _strided([k, k[::-1].copy()], n, 0)
    for i in range(2):
        a = np.float32(g.avg[i].item())
        assert a.view(np.uint32) == m.avg_f32.view(np.uint32), (n, i, float(a), float(m.avg_f32))
    _verify(f"midpoint n={n}", _items(["mid", "mid reversed"], [k, k[::-1].copy()], g, range(2)))


# ---------------------------------------------------------------- exact zeros
def test_single_sample_and_constant_segments():
    """n = 1 and all-equal segments give STD +0.0 (bits) on the strided and ragged paths (the
    FULL / group paths hold 64 PL samples: their all-equal member is in the family above)."""
    vals = np.array([0, 1, 12345, 16_777_217, 0x7FFFFFFF, 0xDFFFFFFF, 0xE0000000, 0xF0000000], np.uint32)
    for begin in (0, 1):
        g = _strided([np.array([v], np.uint32) for v in vals], 1, begin)
        assert np.all(g.std.numpy().view(np.uint32) == 0), g.std
        for i, v in enumerate(vals):
            M.check(g.avg[i].item(), g.std[i].item(), np.array([v], np.uint32), tag=f"n=1 key {v}")
    lens = np.array([1, 200, 1, 1000, 8189, 129, 1], np.int64)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    host = np.repeat(np.array([5, 99_999, 4_000_000_000, 7, 3_000_000_000, 1, 0], np.uint32), lens)
    assert not any(C.sent_to_exact(int(L), False) for L in lens)
    g = ops.segment_stats_ragged(_dev(host), torch.from_numpy(off).to(DEV), None, max_len=8189, cap=0,
                                 mode=ops.STATS_FAST).cpu()
    assert np.all(g.std.numpy().view(np.uint32) == 0), g.std
    for s in range(len(lens)):
        M.check(g.avg[s].item(), g.std[s].item(), host[off[s]:off[s + 1]], tag=f"constant segment {s}")


# ---------------------------------------------------------------- what stays bit-exact
def test_family_exact_mode_and_lane_classes_bit_exact():
    """EXACT mode, and FAST segments of <= 128 samples on the ragged path (lane classes), carry
    computeStats' own AVG / STD bits on the pivot-outlier family too."""
    for n in (1024, 8191):
        fam = C.outlier_family(n)
        g = _strided(list(fam.values()), n, 0, mode=ops.STATS_EXACT)
        _verify(f"EXACT mode n={n}", _items(fam.keys(), fam.values(), g, range(len(fam))), exact=True)
    names, segs = [], []
    for n in (8, 33, 100, 128):
        for nm, k in C.outlier_family(n).items():
            names.append(f"{nm} n={n}")
            segs.append(k)
    lens = np.array([k.size for k in segs], np.int64)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    g = ops.segment_stats_ragged(_dev(np.concatenate(segs)), torch.from_numpy(off).to(DEV), None,
                                 max_len=128, cap=0, mode=ops.STATS_FAST).cpu()
    _verify("lane classes n<=128", _items(names, segs, g, range(len(segs))), exact=True)
