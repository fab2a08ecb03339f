"""GPU: records_bucket_kernel (csrc/records.hip) on streams built for one branch each
(tests/_records_cases.py), against the plain reference retain() (tests/_records_model.py).

That a case takes its branch is proved on the CPU (tests/test_records_model_cpu.py).  Here every
case goes through records_bucket -- counts, lengths, alignment, content (overflowed rings bit for
bit in push order, the others as multisets), buckets disjoint and inside records_bucket_capacity,
nothing written past it -- and through records_stats against oracle.records_stats of the stream
without its invalid records.  There is no tolerance beyond tests/_fastbars.py.

Two assertions tie the device to the layout model: the buckets records_stats flags as reduced
(seg_len < 0) are the model's `reduced` set, and inside a stream and pass the buckets lie in the
order of the model's tiers.  Both follow the constants mirrored in tests/_records_model.py and move
with them: after a change of RB_TINY, RB_COLD, the stage or the LDS budget in records.hip, update
the model, and the CPU claims say which cases need re-aiming."""
import numpy as np
import pytest
import torch

import _records_cases as C
import _records_model as M
import oracle as O
from _fastbars import check_avg_std
from nvidia_resiliency_ext.straggler import ops

pytestmark = pytest.mark.gpu

SENTINEL = -1   # 0xFFFFFFFF: no ns of a case (index + NS0) comes near it
EXTRA = 4096    # words of out_ns past records_bucket_capacity


def _work(case):
    """Work tensors prefilled, out_ns with the sentinel: a run must not pass on what an earlier
    run of the same streams left at the same addresses."""
    n, nstreams = case.recs.shape[0], case.off.size - 1
    G = nstreams * case.nslots
    capacity = ops.records_bucket_capacity(n, nstreams, case.nslots)
    i32 = dict(dtype=torch.int32, device="cuda")
    return capacity, (torch.full((G,), -7, dtype=torch.int64, device="cuda"), torch.full((G,), -7, **i32),
                      torch.full((capacity + EXTRA,), SENTINEL, **i32), torch.full((G,), -7, **i32))


def _device(case):
    return torch.from_numpy(case.recs.view(np.int32)).cuda(), torch.from_numpy(case.off).cuda()


def _reference(case):
    R = M.retain(case.recs, case.off, case.nslots, case.cap)
    lens = np.array([k.size for k in R.kept], np.int64)
    return R, lens


def _check_bucket(case, R, lens):
    d_recs, d_off = _device(case)
    capacity, work = _work(case)
    got = ops.records_bucket(d_recs, d_off, case.nslots, case.cap, out=work)
    seg_off, seg_len, out_ns, counts = (t.cpu().numpy() for t in got)
    assert np.array_equal(counts, R.counts)
    assert np.array_equal(seg_len, lens)
    assert (seg_off % 4 == 0).all()
    assert (seg_off >= 0).all() and (seg_off + seg_len <= capacity).all()
    assert (out_ns[capacity:] == SENTINEL).all(), "written past records_bucket_capacity"
    # pairwise disjoint
    full = np.flatnonzero(lens > 0)
    order = full[np.argsort(seg_off[full], kind="stable")]
    assert (seg_off[order][:-1] + seg_len[order][:-1] <= seg_off[order][1:]).all()
    # content
    gid = np.repeat(np.arange(lens.size), lens)
    within = np.arange(gid.size) - np.repeat(np.cumsum(lens) - lens, lens)
    have = out_ns[seg_off[gid] + within].view(np.uint32)
    want = np.concatenate(R.kept) if R.kept else np.zeros(0, np.uint32)
    ordered = np.repeat(R.counts > lens, lens)  # overflowed rings: push order, bit for bit
    assert ordered.any() == bool(case.cap and (R.counts > case.cap).any())
    assert np.array_equal(have[ordered], want[ordered])
    assert np.array_equal(have[np.lexsort((have, gid))], want[np.lexsort((want, gid))])


def _oracle(case):
    valid = case.recs[:, 0] < case.nslots
    off = np.concatenate([[0], np.cumsum(valid)])[case.off].astype(np.int64)
    recs = np.ascontiguousarray(case.recs[valid])
    ref = O.records_stats(recs, off, case.nslots, cap=case.cap, nthreads=4)
    xm, xs = O.records_moments(recs, off, case.nslots, cap=case.cap, nthreads=4)
    return ref, xm, xs


def _check_stats(case, R, lens, oracle, with_counts):
    d_recs, d_off = _device(case)
    nstreams, nslots, cap = case.off.size - 1, case.nslots, case.cap
    capacity, work = _work(case)
    if not with_counts:
        work = work[:3] + (None,)
    longest = int(np.diff(case.off).max())
    st = ops.records_stats(d_recs, d_off, nslots, cap, max(1, min(longest, cap) if cap else longest),
                           mode=ops.STATS_FAST, bucket=work).cpu()
    ref, xm, xs = oracle
    assert np.array_equal(ref["num"], lens)
    for f in ("num", "min", "max", "med"):
        assert np.array_equal(getattr(st, f).numpy().view(np.int32), ref[f].view(np.int32)), f
    # bit for bit up to 128 records; above, bit for bit or inside the FAST bars
    check_avg_std(st.avg.numpy(), st.std.numpy(), ref, xm, xs, case.name)
    seg_off, seg_len = work[0].cpu().numpy(), work[1].cpu().numpy()
    if with_counts:
        assert np.array_equal(work[3].cpu().numpy(), R.counts)
    assert np.array_equal(np.abs(seg_len), lens)
    # the model's layout, on the device: which buckets the kernel reduced itself, and the order
    # of the others inside their stream and pass (tier by tier, slot order inside a tier)
    for t in range(nstreams):
        for lo, m in M.passes(nslots):
            g = t * nslots + lo + np.arange(m)
            L = M.layout(R.counts[g], cap, m, True)
            assert np.array_equal(seg_len[g] < 0, L.reduced), (case.names[t], lo)
            rest = np.flatnonzero(~L.reduced & (lens[g] > 0))
            assert (seg_off[g][rest] % 4 == 0).all()
            by_model = rest[np.argsort(L.st[rest], kind="stable")]
            by_device = rest[np.argsort(seg_off[g][rest], kind="stable")]
            assert np.array_equal(by_model, by_device), (case.names[t], lo)
            # and exactly as far apart as the model's padded lengths put them
            assert np.array_equal(np.diff(seg_off[g][by_device]), np.diff(L.st[by_device])), (case.names[t], lo)


@pytest.mark.parametrize("i", range(len(C.BUILDERS)), ids=C.IDS)
def test_constructed_streams(i):
    """Every case of tests/_records_cases.py: (a) the five sources of a record, (b) tier edges,
    (c) the stage limit, (d) the ordered walk's step shapes, (e) invalid slots, (f) scan and
    pass edges."""
    case = C.build(i)
    R, lens = _reference(case)
    _check_bucket(case, R, lens)
    oracle = _oracle(case)
    _check_stats(case, R, lens, oracle, with_counts=True)
    if C.BUILDERS[i][0] == "stage":
        _check_stats(case, R, lens, oracle, with_counts=False)
