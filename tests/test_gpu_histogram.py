"""GPU: fixed-bucket duration histograms (segment_histogram.hip) against numpy.

Reference for every case: np.bincount(histograms.bucket_of(retained keys), minlength=240).
Counts are integers, so every comparison is equality; there is no tolerance anywhere.
"""
import numpy as np
import pytest
import torch

import oracle as O
from nvidia_resiliency_ext.straggler import _native, batch, histograms, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
BINS = histograms.BINS
PM = (0, 1, 250, 500, 900, 990, 999, 1000)
WAVE_MAX = 16384  # segment_histogram.hip HIST_WAVE_MAX: length + offset above it takes a workgroup
SENTINEL = -123456789


def _ref(retained):
    return np.bincount(histograms.bucket_of(np.asarray(retained, np.uint32)), minlength=BINS).astype(np.int64)


def _ref_strided(host, nseg, stride, begin, length, cap=0):
    keep = min(length, cap) if cap > 0 else length
    rows = [_ref(host[s * stride + begin + length - keep: s * stride + begin + length]) for s in range(nseg)]
    return np.stack(rows) if rows else np.empty((0, BINS), np.int64)


def _host(t):
    a = t.cpu().numpy()
    return (a.view(np.uint32) if a.dtype == np.int32 else a).astype(np.int64)


def _same(got, ref, what=""):
    got = _host(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (what, bad[:4].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])


def _dev(host_u32):
    return torch.from_numpy(np.ascontiguousarray(host_u32, np.uint32).view(np.int32)).to(DEV)


def _run_strided(host, nseg, stride, begin, length, cap=0):
    num = torch.full((nseg,), -7, dtype=torch.int32, device=DEV)
    out = torch.full((nseg, BINS), SENTINEL, dtype=torch.int32, device=DEV)
    c = ops.segment_histogram_strided(_dev(host), nseg, stride, begin, length, cap=cap, out=out, num=num)
    assert c.data_ptr() == out.data_ptr()
    _same(c, _ref_strided(host, nseg, stride, begin, length, cap), (nseg, stride, begin, length, cap))
    keep = min(length, cap) if cap > 0 else length
    assert num.cpu().tolist() == [keep] * nseg
    return c


# the issue's lengths, and the hand-over from the wave kernel to the workgroup kernel: what
# decides is length + offset in the first 16-byte vector (0..3), so lengths just below WAVE_MAX
# fall on either side of it with the segment's alignment
LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193,
           WAVE_MAX - 4, WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1, 20000]


def _aligned_case(length, begin):
    """Six segments starting `begin` slots into a stride that leaves the next one misaligned."""
    rng = np.random.default_rng(1000 * length + begin)
    stride = length + begin + (int(rng.integers(0, 5)) if begin else 0)
    if begin and stride % 4 == 0:
        stride += 1
    # half clustered (one or two buckets), half spread over many octaves
    host = rng.integers(100_000, 125_000, size=6 * stride, dtype=np.uint32)
    spread = (np.uint64(1) << rng.integers(3, 32, size=3 * stride, dtype=np.uint64)) + \
        rng.integers(0, 1 << 20, size=3 * stride, dtype=np.uint64)
    host[3 * stride:] = np.minimum(spread, np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return host, stride


@pytest.mark.parametrize("length", LENGTHS)
def test_lengths_and_alignment(length):
    for begin in range(4):
        host, stride = _aligned_case(length, begin)
        _run_strided(host, 6, stride, begin, length)


def _edge_keys():
    e = [int(x) for x in histograms.edges_keys()]
    return np.array(e[:BINS] + [x - 1 for x in e[1:]], np.uint32)  # 480 keys


def _values(kind, n, rng):
    if kind == "all_equal":
        return np.full(n, 123_457, np.uint32)
    if kind == "two_values_1_999":
        v = np.full(n, 2_000_000, np.uint32)
        v[rng.choice(n, max(1, n // 1000), replace=False)] = 1_000
        return v
    if kind == "two_values_999_1":
        v = np.full(n, 1_000, np.uint32)
        v[rng.choice(n, max(1, n // 1000), replace=False)] = 2_000_000
        return v
    if kind == "ramp_up":
        return (np.uint32(5_000) + 37 * np.arange(n)).astype(np.uint32)
    if kind == "ramp_down":
        return (np.uint32(5_000) + 37 * np.arange(n)).astype(np.uint32)[::-1].copy()
    if kind == "three_buckets":  # what a real kernel looks like: a few adjacent buckets
        return rng.choice(np.array([100_000, 113_000, 126_000], np.uint32), size=n)
    assert kind == "full_span"  # every u32, wide keys up to 0xFFFFFFFF among them
    v = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    v[rng.choice(n, max(2, n // 8), replace=False)] = rng.integers(
        _native.KEY_WIDE, 1 << 32, size=max(2, n // 8), dtype=np.uint64).astype(np.uint32)
    v[0], v[-1] = 0xFFFFFFFF, 0
    return v


KINDS = ["all_equal", "two_values_1_999", "two_values_999_1", "ramp_up", "ramp_down", "three_buckets",
         "full_span"]


@pytest.mark.parametrize("kind", KINDS)
def test_value_patterns(kind):
    # a wave-kernel length that is no multiple of anything, and a workgroup-kernel length
    for length, begin in ((5000, 1), (8192, 0), (40_001, 2)):
        rng = np.random.default_rng(length)
        stride = length + begin + 1
        host = np.concatenate([np.concatenate([np.zeros(begin, np.uint32), _values(kind, length, rng),
                                               np.zeros(1, np.uint32)]) for _ in range(3)])
        _run_strided(host, 3, stride, begin, length)


def test_every_edge_and_every_edge_minus_one():
    # 241 edges and 241 edges - 1: edge(240) = 2^32 and edge(0) - 1 wrap to the keys 0 and 0xFFFFFFFF
    keys = np.concatenate([_edge_keys(), np.array([0, 0xFFFFFFFF], np.uint32)])
    assert keys.size == 482
    rng = np.random.default_rng(482)
    for begin in range(4):
        stride = keys.size + begin + 1
        host = np.zeros(4 * stride, np.uint32)
        for s in range(4):
            host[s * stride + begin: s * stride + begin + keys.size] = rng.permutation(keys)
        c = _host(_run_strided(host, 4, stride, begin, keys.size))
        # every bucket holds its own lower edge and the key just below the next edge
        assert c.min() >= 1 and c.sum(1).tolist() == [482] * 4


def test_ring_retention():
    R, K, S, cap = 2, 12, 10000, 8192
    ns = synth.synth_matrix(R, K, S, device=DEV)
    num = torch.zeros(R * K, dtype=torch.int32, device=DEV)
    c = ops.segment_histogram_strided(ns.view(-1), R * K, S, 0, S, cap=cap, num=num)
    host = ns.cpu().numpy().view(np.uint32).reshape(-1)
    _same(c, _ref_strided(host, R * K, S, 0, S, cap))
    assert num.cpu().tolist() == [cap] * (R * K)
    assert _host(c).sum(1).tolist() == num.cpu().tolist()


def _ragged_case(rng, lens, aligned16):
    off, parts, pos = [], [], 0
    for n in lens:
        pad = (-pos) % 4 if aligned16 else int(rng.integers(0, 4))
        parts.append(np.full(pad, 777, np.uint32))
        pos += pad
        off.append(pos)
        m = max(n, 0)
        v = rng.integers(50_000, 60_000, size=m, dtype=np.uint32) if rng.integers(0, 2) else \
            rng.integers(0, 1 << 32, size=m, dtype=np.uint64).astype(np.uint32)
        parts.append(v)
        pos += m
    parts.append(np.zeros(8, np.uint32))
    return np.concatenate(parts), np.array(off, np.int64)


MIX = [0, 1, 3, 64, 0, 255, 1000, 4097, 8192, 12345, WAVE_MAX - 3, WAVE_MAX, WAVE_MAX + 1, 20000, 0, 7]


@pytest.mark.parametrize("aligned16", [False, True])
@pytest.mark.parametrize("form", ["seg_len", "offsets"])
def test_ragged(form, aligned16):
    rng = np.random.default_rng(7 + aligned16)
    if form == "seg_len":
        lens = MIX + [-1, 300, -1]  # two skipped segments
        host, off = _ragged_case(rng, lens, aligned16)
        seg_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
        seg_off = torch.from_numpy(off).to(DEV)
    else:  # nseg + 1 offsets, back to back (aligned only if every length is a multiple of 4)
        lens = [(n + 3) // 4 * 4 for n in MIX] if aligned16 else MIX
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        host = rng.integers(1000, 3_000_000, size=int(off[-1]) + 8, dtype=np.uint32)
        seg_len, seg_off, off = None, torch.from_numpy(off).to(DEV), off[:-1]
    nseg = len(lens)
    out = torch.full((nseg, BINS), SENTINEL, dtype=torch.int32, device=DEV)
    num = torch.full((nseg,), -7, dtype=torch.int32, device=DEV)
    ops.segment_histogram_ragged(_dev(host), seg_off, seg_len, max(lens), aligned16=aligned16,
                                 out=out, num=num)
    got, gnum = out.cpu().numpy(), num.cpu().tolist()
    for s, n in enumerate(lens):
        if n < 0:  # skipped: the sentinel row comes back untouched
            assert (got[s] == SENTINEL).all() and gnum[s] == -7, s
        else:      # an empty segment gives zeros
            assert np.array_equal(got[s].view(np.uint32).astype(np.int64),
                                  _ref(host[off[s]: off[s] + n])), (s, n)
            assert gnum[s] == n


def test_ragged_cap():
    rng = np.random.default_rng(11)
    lens, cap = [10, 5000, 9000, 20000, 0], 4999
    host, off = _ragged_case(rng, lens, False)
    c = ops.segment_histogram_ragged(_dev(host), torch.from_numpy(off).to(DEV),
                                     torch.tensor(lens, dtype=torch.int32, device=DEV), max(lens), cap=cap)
    for s, n in enumerate(lens):
        keep = min(n, cap)
        assert np.array_equal(_host(c)[s], _ref(host[off[s] + n - keep: off[s] + n])), s


def test_accumulate():
    rng = np.random.default_rng(5)
    nseg, length = 5, 3001
    a = rng.integers(1000, 3_000_000, size=nseg * length, dtype=np.uint32)
    b = rng.integers(0, 1 << 32, size=nseg * length, dtype=np.uint64).astype(np.uint32)
    out = torch.full((nseg, BINS), SENTINEL, dtype=torch.int32, device=DEV)
    # accumulate = 0 overwrites the sentinel completely
    ops.segment_histogram_strided(_dev(a), nseg, length, 0, length, out=out)
    ra, rb = _ref_strided(a, nseg, length, 0, length), _ref_strided(b, nseg, length, 0, length)
    _same(out, ra)
    ops.segment_histogram_strided(_dev(b), nseg, length, 0, length, out=out, accumulate=True)
    _same(out, ra + rb)
    # a workgroup-kernel segment, and an empty one that leaves the counts as they are
    long_a = rng.integers(1000, 3_000_000, size=30_000, dtype=np.uint32)
    one = torch.full((1, BINS), SENTINEL, dtype=torch.int32, device=DEV)
    ops.segment_histogram_strided(_dev(long_a), 1, 30_000, 0, 30_000, out=one)
    ops.segment_histogram_strided(_dev(long_a), 1, 30_000, 0, 30_000, out=one, accumulate=True)
    ops.segment_histogram_strided(_dev(long_a), 1, 30_000, 0, 0, out=one, accumulate=True)
    _same(one, 2 * _ref(long_a)[None])
    with pytest.raises(ValueError, match="accumulate"):
        ops.segment_histogram_strided(_dev(a), nseg, length, 0, length, accumulate=True)


def test_graph_capture():
    # no allocation and no synchronisation in the call: it can sit in a captured (linear) graph.
    # Two calls, so that both kernels are in it: cap = 8192 takes the wave kernel, none the workgroup's
    nseg, length = 4, 20_000
    ns = torch.zeros(nseg * length, dtype=torch.int32, device=DEV)
    out_w = torch.zeros((nseg, BINS), dtype=torch.int32, device=DEV)
    out_b = torch.zeros((nseg, BINS), dtype=torch.int32, device=DEV)
    num = torch.zeros(nseg, dtype=torch.int32, device=DEV)

    def calls():
        ops.segment_histogram_strided(ns, nseg, length, 0, length, cap=8192, out=out_w, num=num)
        ops.segment_histogram_strided(ns, nseg, length, 0, length, out=out_b)

    calls()  # warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        calls()
    rng = np.random.default_rng(3)
    for _ in range(2):
        host = rng.integers(1000, 3_000_000, size=nseg * length, dtype=np.uint32)
        ns.copy_(_dev(host))
        out_w.fill_(SENTINEL)
        out_b.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        _same(out_w, _ref_strided(host, nseg, length, 0, length, 8192))
        _same(out_b, _ref_strided(host, nseg, length, 0, length))
        assert num.cpu().tolist() == [8192] * nseg


def test_consistent_with_the_quantile_kernels():
    rng = np.random.default_rng(17)
    nseg, length = 6, 4001
    host = rng.integers(1000, 3_000_000, size=nseg * length, dtype=np.uint32)
    host[:length] = 55_555                                # one bucket
    host[length: 2 * length] = _values("full_span", length, rng)  # the open last bucket
    d = _dev(host)
    c = _host(ops.segment_histogram_strided(d, nseg, length, 0, length))
    q = ops.segment_quantiles_strided(d, nseg, length, 0, length, PM).cpu().numpy()
    for s in range(nseg):
        for j, pm in enumerate(PM):
            lo, hi = histograms.quantile_bounds(c[s], pm)
            assert lo <= float(q[j, s]) and (float(q[j, s]) < hi or hi == float("inf")), (s, pm, lo, q[j, s], hi)


def test_matrix_reporter_histograms():
    R, K, S, cap = 4, 6, 700, 512
    ns = synth.synth_matrix(R, K, S, device=DEV)
    rep = batch.MatrixReporter(R, K, cap=cap, device=torch.device(DEV))
    h = rep.histograms(ns, S)
    assert h.dtype == torch.int32 and tuple(h.shape) == (R, K, BINS)
    host = ns.cpu().numpy().view(np.uint32).reshape(R, K, S)
    ref = _ref_strided(host.reshape(-1), R * K, S, 0, S, cap).reshape(R, K, BINS)
    _same(h, ref)
    # the world's histogram per kernel: the retained samples of every rank together
    world = h.sum(0, dtype=torch.int64).cpu().numpy()
    for k in range(K):
        assert np.array_equal(world[k], _ref(host[:, k, S - cap:].reshape(-1))), k
    assert np.array_equal(histograms.merge(*h.cpu().numpy()), world)
    # a second interval added to the first
    h2 = rep.histograms(ns, S, out=h, accumulate=True)
    assert h2.data_ptr() == h.data_ptr()
    _same(h2, 2 * ref)
    # the report is what it was going to be
    res = rep.report(ns, S)
    st = O.matrix_stats(host.reshape(-1), R * K, S, 0, S, cap)
    assert np.array_equal(rep.stats.cpu().num.numpy(), st["num"]) and res is not None
